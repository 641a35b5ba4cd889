"""Contrast-limited adaptive histogram equalisation (pislam_clahe_*: the step between the mesh warp and the pyramid
build) against the integer statement of include/pislam_hip.h, bit for bit.

`ref_clahe` is that statement in numpy int64, independent of the library.  Every GPU comparison covers whole buffers:
`dst` and `luts` are pre-filled with a sentinel, so bytes beyond `width` in a row and between frames must come back
untouched, and the source's row padding and the gaps between its frames hold a byte that is not image content, so a
read that strays into them shows up in a table or a pixel.  Every case runs with the kernels' options both ways
("clahe_combine", "clahe_lut_global"): they must not change a byte."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SENT = 0xEE          # dst and luts pre-fill
PADB = 0x5B          # source padding (rows, gaps between frames, bytes in front of the first frame)
INVALID = -1
CLAHE_FUNCS = ["pislam_clahe_lut_size", "pislam_clahe_luts_batch", "pislam_clahe_apply_batch", "pislam_clahe_batch"]


# ---- the expectation ------------------------------------------------------------------------------------------------
def tile_size(W, H, tiles_x, tiles_y):
    return -(-W // tiles_x), -(-H // tiles_y)


def reflect(i, n):
    return np.where(i < n, i, 2 * (n - 1) - i)


def ref_tables(src, W, H, tiles_x, tiles_y, clip_q8):
    """src: uint8 [B][>= H][>= W] -> (luts uint8 [B][tiles_y][tiles_x][256], clip, res int64 [B][tiles_y][tiles_x]);
    res is excess % 256 of every tile (-1 without clipping)."""
    src = np.asarray(src)[:, :H, :W]
    B = src.shape[0]
    tw, th = tile_size(W, H, tiles_x, tiles_y)
    area = tw * th
    xi, yi = reflect(np.arange(tw * tiles_x), W), reflect(np.arange(th * tiles_y), H)
    assert xi.min() >= 0 and yi.min() >= 0
    E = src[:, yi][:, :, xi].astype(np.int64)
    tile = (np.arange(B)[:, None, None] * tiles_y + (np.arange(th * tiles_y) // th)[None, :, None]) * tiles_x \
        + (np.arange(tw * tiles_x) // tw)[None, None, :]
    h = np.bincount((tile * 256 + E).ravel(), minlength=B * tiles_y * tiles_x * 256).reshape(B, tiles_y, tiles_x, 256).astype(np.int64)
    assert (h.sum(-1) == area).all()
    clip, res = 0, np.full((B, tiles_y, tiles_x), -1, np.int64)
    if clip_q8 > 0:
        clip = max((clip_q8 * area) >> 16, 1)
        excess = np.maximum(h - clip, 0).sum(-1)
        h = np.minimum(h, clip)
        q, res = excess // 256, excess % 256
        step = np.maximum(256 // np.maximum(res, 1), 1)
        v = np.arange(256)
        h = h + q[..., None] + ((res[..., None] > 0) & (v % step[..., None] == 0) & (v // step[..., None] < res[..., None]))
        assert (h.sum(-1) == area).all()
    luts = np.minimum(255, (255 * np.cumsum(h, -1) + (area >> 1)) // area)
    return luts.astype(np.uint8), clip, res


def ref_blend(src, luts, W, H, tiles_x, tiles_y):
    """The blend step alone: src uint8 [B][>= H][>= W], luts uint8 [B][tiles_y][tiles_x][256] (any bytes) -> [B][H][W]."""
    src = np.asarray(src)[:, :H, :W]
    B = src.shape[0]
    L = np.asarray(luts).astype(np.int64)
    tw, th = tile_size(W, H, tiles_x, tiles_y)

    def axis(n, t, tiles):
        f = 2 * np.arange(n, dtype=np.int64) - t
        t1 = f // (2 * t)                                   # numpy's // is a floor division
        w2 = f - 2 * t * t1
        assert (w2 >= 0).all() and (w2 < 2 * t).all() and t1.min() >= -1 and t1.max() <= tiles - 1
        return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), 2 * t - w2, w2

    tx1, tx2, wx1, wx2 = [a[None, None, :] for a in axis(W, tw, tiles_x)]
    ty1, ty2, wy1, wy2 = [a[None, :, None] for a in axis(H, th, tiles_y)]
    b, v = np.arange(B)[:, None, None], src.astype(np.int64)
    S = wy1 * (wx1 * L[b, ty1, tx1, v] + wx2 * L[b, ty1, tx2, v]) + wy2 * (wx1 * L[b, ty2, tx1, v] + wx2 * L[b, ty2, tx2, v])
    D = 4 * tw * th
    assert S.max() + (D >> 1) < 1 << 32
    out = (S + (D >> 1)) // D
    assert out.min() >= 0 and out.max() <= 255
    return np.ascontiguousarray(out.astype(np.uint8))      # (fancy indexing may leave another memory order)


def ref_clahe(src, W, H, tiles_x, tiles_y, clip_q8):
    """-> (out uint8 [B][H][W], luts uint8 [B][tiles_y][tiles_x][256], clip)"""
    luts, clip, _ = ref_tables(src, W, H, tiles_x, tiles_y, clip_q8)
    return ref_blend(src, luts, W, H, tiles_x, tiles_y), luts, clip


def random_frames(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W), dtype=np.uint8)


def low_contrast(B, H, W, seed):
    return ((random_frames(B, H, W, seed) // 32) * 3 + 100).astype(np.uint8)


def mixed_pair(H, W, seed):
    """Frame 0 uniform random, frame 1 low-contrast."""
    return np.concatenate([random_frames(1, H, W, seed), low_contrast(1, H, W, seed + 1)])


# ---- CPU: declarations and the expectation's anchors ----------------------------------------------------------------
def test_clahe_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for f in CLAHE_FUNCS:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % f, code), f"{f} is not declared in include/pislam_hip.h"
    assert re.search(r"typedef struct pislam_clahe_params \{[^}]*\} pislam_clahe_params;", code)
    from pislam_amd import capi, frontend
    for f in CLAHE_FUNCS:
        assert f in capi.SYMBOLS
    assert [n for n, _ in capi.ClaheParams._fields_] == ["width", "height", "tiles_x", "tiles_y", "clip_q8"]
    for m in ("luts", "apply", "__call__"):
        assert callable(getattr(frontend.Clahe, m))
    lib = capi.load()

    def size(*p):
        return lib.pislam_clahe_lut_size(ctypes.byref(capi.ClaheParams(*p)))

    assert size(640, 480, 8, 8, 768) == 8 * 8 * 256 and size(1, 1, 1, 1, 0) == 256 and size(4096, 4096, 4, 4, 65535) == 16 * 256
    assert size(37, 23, 4, 3, 768) == 12 * 256 and size(32, 32, 32, 32, 1) == 1024 * 256 and size(2048, 512, 1, 1, 0) == 256
    for bad in ((0, 8, 1, 1, 768), (8, 0, 1, 1, 768), (4097, 8, 8, 1, 768), (8, 4097, 1, 8, 768), (5, 8, 6, 1, 768), (8, 5, 1, 6, 768),
                (64, 64, 33, 1, 768), (64, 64, 1, 33, 768), (64, 64, 0, 1, 768), (64, 64, 1, 0, 768), (64, 64, -1, 1, 768),
                (4096, 4096, 2, 2, 768), (2049, 512, 1, 1, 768), (64, 64, 8, 8, -1), (64, 64, 8, 8, 65536)):
        assert size(*bad) == 0, bad
    assert lib.pislam_clahe_lut_size(None) == 0


def test_ref_clahe_anchors():
    """The expectation itself, independent of the library."""
    # a constant frame of value v comes out as lut[v] everywhere: S is an exact multiple of D
    for (W, H, tx, ty, q8) in ((37, 23, 4, 3, 768), (64, 48, 8, 8, 768), (19, 7, 10, 4, 40)):
        src = np.full((1, H, W), 93, np.uint8)
        out, luts, _ = ref_clahe(src, W, H, tx, ty, q8)
        assert (luts == luts[0, 0, 0]).all() and (out == luts[0, 0, 0, 93]).all()
    # one tile without clipping is global histogram equalisation
    src = random_frames(2, 23, 37, 1) // 3
    out, luts, clip = ref_clahe(src, 37, 23, 1, 1, 0)
    assert clip == 0
    for b in range(2):
        cdf = np.cumsum(np.bincount(src[b].ravel(), minlength=256))
        ge = np.minimum(255, (255 * cdf + (37 * 23) // 2) // (37 * 23))
        assert (luts[b, 0, 0] == ge).all() and (out[b] == ge[src[b]]).all()
    # a 256 x 16 ramp, one tile, minimal clip: every bin is cut to 1 and refilled evenly, the table is the identity +- 1
    ramp = np.tile(np.arange(256, dtype=np.uint8), (16, 1))[None]
    out, luts, clip = ref_clahe(ramp, 256, 16, 1, 1, 1)
    assert clip == 1 and np.abs(out.astype(int) - ramp.astype(int)).max() <= 1
    # a low-contrast frame gains contrast
    dim = low_contrast(1, 48, 64, 2)
    out, _, clip = ref_clahe(dim, 64, 48, 8, 8, 768)
    assert clip == max((768 * 48) >> 16, 1) and out.std() > dim.std()
    # the residual's closed form against OpenCV's loop
    for res in (0, 1, 2, 3, 42, 64, 127, 128, 129, 200, 255):
        h = np.zeros(256, np.int64)
        if res:
            step, left, i = max(256 // res, 1), res, 0
            while i < 256 and left > 0:
                h[i] += 1
                i += step
                left -= 1
        v = np.arange(256)
        step = max(256 // max(res, 1), 1)
        assert (h == ((res > 0) & (v % step == 0) & (v // step < res))).all() and h.sum() == res


# ---- GPU -------------------------------------------------------------------------------------------------------------
VARIANTS = ((1, 0), (0, 1))          # ("clahe_combine", "clahe_lut_global"): the defaults, and both alternatives


class Device:
    """Flat device buffers around a CLAHE call: frames at an odd offset, padded rows, a gap between frames."""

    def __init__(self, ctx):
        import torch
        from pislam_amd import capi
        self.torch, self.ctx, self.lib, self.capi = torch, ctx, ctx.lib, capi

    def params(self, W, H, tx, ty, q8):
        return self.capi.ClaheParams(W, H, tx, ty, q8)

    def source(self, frames, W, pad, gap, off):
        """-> (device tensor, vstep, stride): frames uint8 [B][H][W] laid out with `pad`, `gap` and `off` bytes of PADB"""
        B, H = frames.shape[:2]
        vs = W + pad
        stride = H * vs + gap
        host = np.full(off + B * stride, PADB, np.uint8)
        np.lib.stride_tricks.as_strided(host[off:], (B, H, vs), (stride, vs, 1))[:, :, :W] = frames[:, :, :W]
        return self.torch.from_numpy(host).cuda(), vs, stride

    def expect(self, want, W, vs, stride, off, fill):
        B, H = want.shape[:2]
        host = np.full(off + B * stride, fill, np.uint8)
        np.lib.stride_tricks.as_strided(host[off:], (B, H, vs), (stride, vs, 1))[:, :, :W] = want
        return host

    def same(self, got, want, what):
        got = got.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"

    def options(self, combine, lut_global):
        self.ctx.set_option("clahe_combine", combine)
        self.ctx.set_option("clahe_lut_global", lut_global)

    def run(self, shape, frames, want_out, want_luts, pad=0, dpad=0, gap=0, off=0, in_place=False, given_luts=None):
        """pislam_clahe_batch (or, with given_luts, pislam_clahe_apply_batch) under every variant; whole dst and luts
        buffers against the expectation."""
        torch = self.torch
        W, H, tx, ty, q8 = shape
        p = self.params(*shape)
        B = frames.shape[0]
        nl = tx * ty * 256
        for combine, lut_global in VARIANTS:
            src, svs, sstride = self.source(frames, W, pad, gap, off)
            if in_place:
                dst, dvs, dstride, fill = src, svs, sstride, PADB
            else:
                dvs = W + dpad
                dstride = H * dvs + (gap + 3 if gap else 0)
                dst, fill = torch.full((off + B * dstride,), SENT, dtype=torch.uint8, device="cuda"), SENT
            luts = torch.full((3 + B * nl + 5,), SENT, dtype=torch.uint8, device="cuda")
            if given_luts is not None:
                luts[3:3 + B * nl] = torch.from_numpy(given_luts.reshape(-1)).cuda()
            self.options(combine, lut_global)
            try:
                if given_luts is None:
                    rc = self.lib.pislam_clahe_batch(self.ctx.h, ctypes.byref(p), src.data_ptr() + off, svs, sstride,
                                                     dst.data_ptr() + off, dvs, dstride, B, luts.data_ptr() + 3)
                else:
                    rc = self.lib.pislam_clahe_apply_batch(self.ctx.h, ctypes.byref(p), src.data_ptr() + off, svs, sstride,
                                                           luts.data_ptr() + 3, dst.data_ptr() + off, dvs, dstride, B)
            finally:
                self.options(1, 0)
            assert rc == 0, self.lib.pislam_last_error(self.ctx.h)
            self.ctx.synchronize()
            tag = f"{shape} combine={combine} lut_global={lut_global}"
            wl = np.full(3 + B * nl + 5, SENT, np.uint8)
            wl[3:3 + B * nl] = want_luts.reshape(-1)
            self.same(luts, wl, "luts " + tag)
            self.same(dst, self.expect(want_out, W, dvs, dstride, off, fill), "dst " + tag)


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    return Device(gpu_ctx)


MATRIX = [(37, 23, 4, 3, 768), (64, 48, 8, 8, 768), (5, 5, 5, 5, 256), (1, 1, 1, 1, 0), (33, 20, 2, 7, 0), (100, 60, 3, 2, 768),
          (100, 60, 3, 2, 65535), (19, 7, 10, 4, 40), (131, 67, 32, 32, 5000), (640, 480, 8, 8, 768)]
# pad (source rows), dpad (destination rows), gap between frames, offset of the first frame
LAYOUTS = [(5, 2, 7, 3), (0, 0, 0, 0), (3, 3, 1, 1), (2, 1, 3, 1), (7, 0, 0, 2), (0, 4, 5, 0), (1, 1, 0, 0), (9, 2, 2, 3), (3, 0, 6, 1),
           (0, 0, 0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(MATRIX)), ids=["x".join(map(str, s)) for s in MATRIX])
def test_gpu_matrix_against_ref_clahe(dev, k):
    """Batch 2: frame 0 uniform random, frame 1 low-contrast; tables and output bit-equal.  The layouts give padded
    source rows, a destination vstep that differs from the source's and gaps between frames; the workload's own shape
    runs once, plain."""
    shape = MATRIX[k]
    W, H, tx, ty, q8 = shape
    pad, dpad, gap, off = LAYOUTS[k]
    frames = mixed_pair(H, W, 10 + k)
    out, luts, clip = ref_clahe(frames, W, H, tx, ty, q8)
    if shape == (100, 60, 3, 2, 768):
        assert clip == 11
    dev.run(shape, frames, out, luts, pad=pad, dpad=dpad, gap=gap, off=off)


def residual_cases():
    """One-tile frames (W x 1) whose excess % 256 hits 0, 1, 2..128 (step >= 2), > 128 (step 1) and 255: constant frames
    have excess = area - clip, two-valued ones with both bins above the clip area - 2 * clip."""
    cases = []
    for W, two in ((257, False), (258, False), (321, False), (201, False), (256, False), (300, True), (258, True), (513, True)):
        f = np.full((1, 1, W), 77, np.uint8)
        if two:
            f[0, 0, ::2] = 200
        cases.append(((W, 1, 1, 1, 1), f))
    return cases


@pytest.mark.gpu
def test_gpu_residual_coverage(dev):
    seen = set()
    for shape, frames in residual_cases():
        W, H, tx, ty, q8 = shape
        luts, clip, res = ref_tables(frames, W, H, tx, ty, q8)
        assert clip == 1
        r = int(res[0, 0, 0])
        seen.add("0" if r == 0 else "1" if r == 1 else "255" if r == 255 else "step>=2" if r <= 128 else "step1")
        dev.run(shape, frames, ref_blend(frames, luts, W, H, tx, ty), luts, pad=1, off=1)
    assert seen == {"0", "1", "step>=2", "step1", "255"}, seen


def hand_made_tables(B, tx, ty, kind, seed):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (B, ty, tx, 256), dtype=np.uint8)
    t = np.zeros((B, ty, tx, 256), np.uint8)
    if kind == "columns":                                   # neighbouring tiles all 0 against all 255
        t[:, :, 1::2] = 255
    else:                                                   # a checkerboard of 0 / 255 tables
        t[:, (np.indices((ty, tx)).sum(0) & 1).astype(bool)] = 255
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(37, 23, 4, 3), (64, 48, 8, 8), (4096, 8, 4, 1)], ids=lambda s: "x".join(map(str, s)))
def test_gpu_apply_with_hand_made_tables(dev, shape):
    """pislam_clahe_apply_batch alone with tables that are not monotone: the exact division and the clamps without the
    histogram."""
    W, H, tx, ty = shape
    frames = random_frames(2, H, W, 30)
    for j, kind in enumerate(("random", "columns", "checker")):
        tables = hand_made_tables(2, tx, ty, kind, 31 + j)
        want = ref_blend(frames, tables, W, H, tx, ty)
        if kind != "random":
            assert want.min() == 0 and want.max() == 255 and len(np.unique(want)) > 8
        dev.run(shape + (0,), frames, want, tables, pad=3 * (j & 1), dpad=j, gap=j, off=j, given_luts=tables)


@pytest.mark.gpu
def test_gpu_in_place(dev):
    """dst == src (same pointer, vstep and stride) gives the bytes of the out-of-place call, for pislam_clahe_batch and
    for pislam_clahe_apply_batch; the source's padding stays as it was."""
    for shape in ((37, 23, 4, 3, 768), (64, 48, 8, 8, 768), (100, 60, 3, 2, 768)):
        W, H, tx, ty, q8 = shape
        frames = mixed_pair(H, W, 40)
        out, luts, _ = ref_clahe(frames, W, H, tx, ty, q8)
        dev.run(shape, frames, out, luts, pad=5, gap=3, off=1, in_place=True)
        tables = hand_made_tables(2, tx, ty, "random", 41)
        dev.run(shape, frames, ref_blend(frames, tables, W, H, tx, ty), tables, pad=2, gap=1, off=3, in_place=True, given_luts=tables)


@pytest.mark.gpu
def test_gpu_batch_past_65535(dev):
    """70000 frames of 8 x 4 at 2 x 2 tiles: more than one grid dimension holds.  Frame b is distinct frame b % 251 (the
    expectation is computed once per distinct frame), so frames 65535.. differ from frames 0.. at the same grid index."""
    B, shape = 70000, (8, 4, 2, 2, 768)
    distinct = random_frames(251, 4, 8, 50)
    distinct[1::2] = (distinct[1::2] // 32) * 3 + 100
    out, luts, _ = ref_clahe(distinct, *shape)
    pick = np.arange(B) % 251
    dev.run(shape, distinct[pick], out[pick], luts[pick], pad=1, gap=2, off=1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4096, 16, 32, 1, 768), (16, 4096, 1, 32, 768)], ids=lambda s: "x".join(map(str, s)))
def test_gpu_coordinate_limit(dev, shape):
    W, H = shape[:2]
    frames = mixed_pair(H, W, 51)
    out, luts, _ = ref_clahe(frames, *shape)
    dev.run(shape, frames, out, luts, pad=3, dpad=1, gap=1, off=1)


@pytest.mark.gpu
def test_gpu_largest_tile(dev):
    """2048 x 512 with one tile: area == 2^20 exactly.  Frame 0 is constant (one bin holds 2^20), frame 1 random."""
    shape = (2048, 512, 1, 1, 768)
    frames = random_frames(2, 512, 2048, 52)
    frames[0] = 201
    luts, clip, res = ref_tables(frames, *shape)
    assert clip == (768 << 20) >> 16
    dev.run(shape, frames, ref_blend(frames, luts, 2048, 512, 1, 1), luts)
    out0, luts0, _ = ref_clahe(frames, 2048, 512, 1, 1, 0)
    dev.run((2048, 512, 1, 1, 0), frames, out0, luts0, pad=4)


@pytest.mark.gpu
def test_gpu_strides_past_4_gib(dev):
    """Two frames whose src_stride and dst_stride put frame 1 beyond 4 GiB (allocated in one piece, as
    test_after_match_limits.py does): only the frames' own bytes are set and looked at."""
    torch = dev.torch
    shape = (64, 48, 8, 8, 768)
    W, H, tx, ty, q8 = shape
    stride = (1 << 32) + 12345
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * (stride + H * W) + (1 << 30):
        pytest.skip("two buffers of 4 GiB do not fit the free device memory")
    frames = mixed_pair(H, W, 53)
    out, luts, _ = ref_clahe(frames, *shape)
    src = dst = lut = None
    try:
        src = torch.empty((stride + H * W,), dtype=torch.uint8, device="cuda")
        dst = torch.empty((stride + H * W,), dtype=torch.uint8, device="cuda")
        lut = torch.full((2 * tx * ty * 256,), SENT, dtype=torch.uint8, device="cuda")
        for b in range(2):
            src[b * stride:b * stride + H * W] = torch.from_numpy(frames[b].reshape(-1)).cuda()
            dst[b * stride:b * stride + H * W + 64 * (1 - b)] = SENT
        p = dev.params(*shape)
        rc = dev.lib.pislam_clahe_batch(dev.ctx.h, ctypes.byref(p), src.data_ptr(), W, stride, dst.data_ptr(), W, stride, 2,
                                        lut.data_ptr())
        assert rc == 0, dev.lib.pislam_last_error(dev.ctx.h)
        dev.ctx.synchronize()
        assert (lut.cpu().numpy().reshape(luts.shape) == luts).all()
        for b in range(2):
            assert (dst[b * stride:b * stride + H * W].cpu().numpy().reshape(H, W) == out[b]).all(), b
        assert (dst[H * W:H * W + 64].cpu().numpy() == SENT).all()
    finally:
        src = dst = lut = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_gpu_validation(dev):
    """Every limit of the header, overlaps, host pointers and NULLs: PISLAM_ERR_INVALID with the sentinel-filled outputs
    untouched.  batch == 0 returns PISLAM_OK after the checks of p, batch and the steps, NULL data pointers accepted."""
    torch, lib, ctx = dev.torch, dev.lib, dev.ctx
    W, H, tx, ty, q8, B = 40, 24, 4, 3, 768, 2
    nl = tx * ty * 256
    src = torch.full((B * H * W + 64,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((B * H * W + 64 + B * nl,), SENT, dtype=torch.uint8, device="cuda")
    luts = torch.full((B * nl,), SENT, dtype=torch.uint8, device="cuda")
    host = np.zeros(B * H * W + B * nl, np.uint8)

    def call(fn="batch", p=(W, H, tx, ty, q8), s=None, svs=W, sst=H * W, d=None, dvs=W, dst_=H * W, l=None, B=B, null_p=False):
        s = src.data_ptr() if s is None else s
        d = dst.data_ptr() if d is None else d
        l = luts.data_ptr() if l is None else l
        pp = None if null_p else ctypes.byref(dev.params(*p))
        if fn == "batch":
            return lib.pislam_clahe_batch(ctx.h, pp, s, svs, sst, d, dvs, dst_, B, l)
        if fn == "luts":
            return lib.pislam_clahe_luts_batch(ctx.h, pp, s, svs, sst, B, l)
        return lib.pislam_clahe_apply_batch(ctx.h, pp, s, svs, sst, l, d, dvs, dst_, B)

    for fn in ("batch", "luts", "apply"):
        assert call(fn) == 0, lib.pislam_last_error(ctx.h)
    ctx.synchronize()
    dst.fill_(SENT)
    luts.fill_(SENT)
    bad = [dict(p=(0, H, 1, ty, q8)), dict(p=(W, 0, tx, 1, q8)), dict(p=(4097, H, tx, ty, q8)), dict(p=(W, 4097, tx, ty, q8)),
           dict(p=(W, H, 0, ty, q8)), dict(p=(W, H, tx, 0, q8)), dict(p=(W, H, 33, ty, q8)), dict(p=(W, H, tx, 25, q8)),
           dict(p=(3, H, 4, ty, q8)), dict(p=(4096, 4096, 2, 2, q8)), dict(p=(W, H, tx, ty, -1)), dict(p=(W, H, tx, ty, 65536)),
           dict(null_p=True), dict(svs=W - 1), dict(B=-1), dict(s=host.ctypes.data), dict(l=host.ctypes.data), dict(s=0), dict(l=0),
           dict(l=src.data_ptr() + 8),                                                # luts inside src
           dict(s=luts.data_ptr() + nl - 1, B=1)]                                    # (one frame) src begins on luts' last byte
    bad_dst = [dict(dvs=W - 1), dict(d=host.ctypes.data), dict(d=0),
               dict(l=dst.data_ptr() + 16),                                           # luts inside dst
               dict(l=dst.data_ptr() + B * H * W - 1),                                # luts begins on dst's last byte
               dict(d=src.data_ptr() + 1),                                            # dst shifted by one byte against src
               dict(d=src.data_ptr(), dvs=W + 1), dict(d=src.data_ptr(), dst_=H * W + 1),   # the same pointer, other steps
               dict(d=src.data_ptr() + B * H * W - 1)]                                # dst begins on src's last byte
    for fn in ("batch", "luts", "apply"):
        for kw in bad + (bad_dst if fn != "luts" else []):
            assert call(fn, **kw) == INVALID, (fn, kw)
            assert lib.pislam_last_error(ctx.h)
    for fn in ("batch", "luts", "apply"):
        assert call(fn, B=0) == 0 and call(fn, B=0, s=0, d=0, l=0) == 0
        assert call(fn, B=0, p=(W, H, 33, ty, q8)) == INVALID and call(fn, B=0, svs=W - 1) == INVALID
    assert lib.pislam_ctx_set_option(ctx.h, b"clahe_combine", 2) == INVALID
    assert lib.pislam_ctx_set_option(ctx.h, b"clahe_lut_global", -1) == INVALID
    ctx.synchronize()
    assert (dst.cpu().numpy() == SENT).all() and (luts.cpu().numpy() == SENT).all() and (src.cpu().numpy() == 7).all()
    # touching ranges are no overlap: src, then dst, then luts in one allocation
    one = torch.full((2 * B * H * W + B * nl,), 7, dtype=torch.uint8, device="cuda")
    assert call(s=one.data_ptr(), d=one.data_ptr() + B * H * W, l=one.data_ptr() + 2 * B * H * W) == 0
    ctx.synchronize()
    want, wl, _ = ref_clahe(np.full((B, H, W), 7, np.uint8), W, H, tx, ty, q8)
    got = one.cpu().numpy()
    assert (got[:B * H * W] == 7).all() and (got[B * H * W:2 * B * H * W] == want.reshape(-1)).all()
    assert (got[2 * B * H * W:] == wl.reshape(-1)).all()
    # the Python class checks shapes itself
    from pislam_amd import capi
    from pislam_amd.frontend import Clahe
    with pytest.raises(capi.PislamError):
        Clahe(W, H, tiles=(33, 1), ctx=ctx)
    cl = Clahe(W, H, tiles=(tx, ty), ctx=ctx)
    assert cl.lut_size == nl
    with pytest.raises(ValueError):
        cl(torch.zeros((B, H + 1, W), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        cl(torch.zeros((B, H, W), dtype=torch.uint8, device="cuda"), luts=torch.zeros((B, ty, tx, 255), dtype=torch.uint8, device="cuda"))


@pytest.mark.gpu
def test_gpu_frontend_class(dev):
    """frontend.Clahe: luts + apply == __call__ == the reference, on views with padded rows, in place too."""
    torch = dev.torch
    from pislam_amd.frontend import Clahe
    W, H, B = 70, 37, 3
    frames = np.concatenate([mixed_pair(H, W, 60), low_contrast(1, H, W, 62)])
    want, wl, _ = ref_clahe(frames, W, H, 8, 8, 768)
    cl = Clahe(W, H, ctx=dev.ctx)
    assert cl.tiles == (8, 8) and cl.clip_q8 == 768 and cl.lut_size == 64 * 256
    buf = torch.full((B, H, W + 6), PADB, dtype=torch.uint8, device="cuda")
    buf[:, :, :W] = torch.from_numpy(frames).cuda()
    view = buf[:, :, :W]
    out = cl(view)
    assert tuple(out.shape) == (B, H, W) and tuple(cl.last_luts.shape) == (B, 8, 8, 256)
    tables = cl.luts(view)
    out2 = cl.apply(view, tables)
    assert cl(view, out=view) is view                       # in place
    dev.ctx.synchronize()
    assert (out.cpu().numpy() == want).all() and (out2.cpu().numpy() == want).all()
    assert (tables.cpu().numpy() == wl).all() and (cl.last_luts.cpu().numpy() == wl).all()
    got = buf.cpu().numpy()
    assert (got[:, :, :W] == want).all() and (got[:, :, W:] == PADB).all()


@pytest.mark.gpu
def test_gpu_warp_clahe_then_pyramid_build(dev):
    """Warp -> Clahe -> PyramidBuilder (blur on) == PyramidBuilder on ref_clahe(ref_warp(...)) uploaded, on every byte
    the build defines."""
    import torch
    from pislam_amd.frontend import Clahe, PyramidBuilder, Warp
    from test_prep import build_defined_mask
    from test_warp import affine_mesh, ref_warp
    W, H, SW, SH, B, steps, lc = 96, 80, 110, 101, 2, (2, 1), 3
    src = low_contrast(B, SH, SW, 70)
    mesh = affine_mesh(W, H, lc, (260, 10, 300), (-8, 270, 1200), jitter=200, seed=7)
    warp = Warp(*mesh, W, H, SW, SH, lc, ctx=dev.ctx)
    clahe = Clahe(W, H, ctx=dev.ctx)
    pb = PyramidBuilder(W, H, steps, blur=True, ctx=dev.ctx)
    pyr = [torch.full((B, pb.rows, pb.vstep), 0, dtype=torch.uint8, device="cuda") for _ in range(2)]
    eq = clahe(warp(torch.from_numpy(src).cuda()))
    pb(eq, pyr[0])
    want, _, _ = ref_clahe(ref_warp(*mesh, lc, W, H, src, SW, SH, 0), W, H, 8, 8, 768)
    pb(torch.from_numpy(want).cuda(), pyr[1])
    dev.ctx.synchronize()
    assert (eq.cpu().numpy() == want).all() and want.std() > src.std()
    mask = build_defined_mask(pb, steps)
    a, b = pyr[0].cpu().numpy(), pyr[1].cpu().numpy()
    assert mask.any() and (a[:, mask] == b[:, mask]).all()
    warp.close()


@pytest.mark.gpu
def test_gpu_clahe_is_hipgraph_capturable(gpu_ctx):
    """No workspace, no host round trip: both kernels captured on a side stream of a fresh context without a warm-up
    call, replayed twice with fresh sources in the same tensor."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import Clahe
    W, H, B = 70, 37, 2
    side = torch.cuda.Stream(torch.device("cuda:0"))
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        clahe = Clahe(W, H, tiles=(4, 3), clip_q8=512, ctx=ctx)
        src = torch.zeros((B, H, W), dtype=torch.uint8, device="cuda")
        dst = torch.full((B, H, W + 3), SENT, dtype=torch.uint8, device="cuda")
        luts = torch.full((B, 3, 4, 256), SENT, dtype=torch.uint8, device="cuda")
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            clahe(src, dst[:, :, :W], luts)
        for seed in (80, 82):
            frames = mixed_pair(H, W, seed)
            src.copy_(torch.from_numpy(frames).cuda())
            dst.fill_(SENT)
            luts.fill_(SENT)
            g.replay()
            side.synchronize()
            want, wl, _ = ref_clahe(frames, W, H, 4, 3, 512)
            got = dst.cpu().numpy()
            assert (got[:, :, :W] == want).all() and (got[:, :, W:] == SENT).all() and (luts.cpu().numpy() == wl).all()
        ctx.close()
