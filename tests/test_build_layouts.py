"""pislam_pyramid_build_batch and the stand-alone gaussian5x5 / bilinear7_8 / bilinear13_16 on the layouts their
signatures allow: padded frame rows, gaps between frames and between pyramids, bases that are not 16- or 4-byte aligned, a
vstep that is no multiple of 16, batches past 65535, strides past 4 GiB and a hipGraph replay.

The kernels choose their code paths from exactly these values (pislam_prep_kernels.h, pislam_prep_plan.h): the Gaussian
stages a tile with 16-byte loads, dwords or bytes, per frame; the 4-block reduction kernel needs aligned, wide enough rows or
the one-lane kernel runs; the one-launch chain needs the 4-block kernel on every level; stores and the margin pass switch
between vectors, dwords and bytes.  PyramidBuilder always passes the contiguous layout at torch-aligned bases, so the other
modules reach one path per kernel.

`ref_build` restates a whole build in numpy integers — no project kernel — and one CPU test anchors it on the oracle's
gaussian5x5, bilinear7_8 and bilinear13_16 in sequence.  Every GPU comparison is bit-exact and covers the whole destination
allocation: the bytes a build defines equal the reference, every other byte (in front of, between and behind the pyramids,
beyond the margins) keeps the sentinel, and every source byte that is not a pixel holds a poison value no frame contains.
The path rules are restated below in a few lines each, and `test_matrix_covers_every_path` asserts from them, without a
GPU, that the case matrix reaches every path."""
import ctypes
import functools

import numpy as np
import pytest

SENT = 0xEE                        # destination pre-fill
POISON = 0x5B                      # every source byte that is not a pixel; no frame holds it
BLUR, CLEAN, CHECK = 1, 2, 4       # PISLAM_BUILD_*
INVALID = -1
PLAIN = (0, 0, 0)
F7 = np.array([238, 201, 165, 128, 91, 55, 18], np.int64)
F13 = np.array([226, 167, 108, 49, 246, 187, 128, 69, 10, 207, 138, 89, 30], np.int64)


def cdiv(a, b):
    return -(-a // b)


def block(step):
    """step code -> (N, M): N x N source pixels become M x M"""
    return (8, 7) if step == 1 else (16, 13)


# ---- 1. the expectation ----------------------------------------------------------------------------------------------
def ref_layout(width, height, steps, vstep_min=0):
    """pislam_pyramid_layout restated -> ([(w, h, row0)], vstep, rows): sizes round down, a slot keeps the rows of the
    larger block padding and every row the reduction into it writes."""
    w, h, row, maxcols, levels = width, height, 0, width, []
    for l in range(len(steps) + 1):
        written = 0
        if l:
            N, M = block(steps[l - 1])
            written, maxcols = cdiv(h, N) * M, max(maxcols, cdiv(w, N) * M)
            w, h = w * M // N, h * M // N
        assert w >= 3 and h >= 3
        levels.append((w, h, row))
        row += max(cdiv(h, 16) * 16, written)
    return levels, max(vstep_min, cdiv(maxcols, 16) * 16), row


def rshr8(a):
    return (a + 128) >> 8


def ref_reduce(src, w, h, step):
    """One 7/8 or 13/16 reduction of the w x h image at the top left of `src` (which holds the block padding too):
    whole M x M output blocks, uint8 [nby * M][nbx * M]."""
    N, M = block(step)
    F = F7 if M == 7 else F13
    k = np.arange(M)
    s = k if M == 7 else k + (k > 3) + (k > 8)           # 13/16: source columns and rows 4 and 10 of a block start no tap pair
    nbx, nby = cdiv(w, N), cdiv(h, N)
    xs = (np.arange(nbx)[:, None] * N + s[None]).ravel()
    ys = (np.arange(nby)[:, None] * N + s[None]).ravel()
    fx0, fx1 = np.tile(F, nbx)[None], np.tile(F[::-1], nbx)[None]
    fy0, fy1 = np.tile(F, nby)[:, None], np.tile(F[::-1], nby)[:, None]
    a = np.asarray(src).astype(np.int64)
    assert ys[-1] + 1 < a.shape[0] and xs[-1] + 1 < a.shape[1]
    top = rshr8(a[ys][:, xs] * fx0 + a[ys][:, xs + 1] * fx1)
    bot = rshr8(a[ys + 1][:, xs] * fx0 + a[ys + 1][:, xs + 1] * fx1)
    out = rshr8(top * fy0 + bot * fy1)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


class Plan:
    """The level table of one shape; `vstep_add` widens the rows beyond what the layout asks for."""

    def __init__(self, width, height, steps, vstep_min=0, vstep_add=0):
        self.width, self.height, self.steps = width, height, tuple(steps)
        self.levels, vstep, self.rows = ref_layout(width, height, steps, vstep_min)
        self.vstep = vstep + vstep_add
        self.n = len(self.levels)

    def slot(self, l):
        return (self.levels[l + 1][2] if l + 1 < self.n else self.rows) - self.levels[l][2]

    def written(self, l):
        """(columns, rows) the build rewrites in level l's slot: the frame, or whole output blocks."""
        if l == 0:
            return self.width, self.height
        N, M = block(self.steps[l - 1])
        return cdiv(self.levels[l - 1][0], N) * M, cdiv(self.levels[l - 1][1], N) * M

    def margin(self, l):
        """(columns, rows) of level l's slot that the build defines: the rewritten rectangle plus 32 columns to the right
        and 16 rows below, clipped to the row and the slot (include/pislam_hip.h)."""
        ww, wh = self.written(l)
        return min(self.vstep, ww + 32), min(self.slot(l), wh + 16)


def ref_build(frame, plan, blur=True):
    """One frame -> (image uint8 [rows][vstep], mask of the bytes the build defines); undefined bytes are 0 here."""
    from pislam_amd import synth
    img = np.zeros((plan.rows, plan.vstep), np.uint8)
    mask = np.zeros(img.shape, bool)
    w, h, r0 = plan.levels[0]
    img[r0:r0 + h, :w] = synth.gaussian5x5(frame[:h, :w]) if blur else frame[:h, :w]
    for l in range(plan.n):
        w, h, r0 = plan.levels[l]
        cols, rows = plan.margin(l)
        mask[r0:r0 + rows, :cols] = True
        if l + 1 < plan.n:
            N, _ = block(plan.steps[l])
            assert mask[r0:r0 + cdiv(h, N) * N, :cdiv(w, N) * N].all()          # a reduction reads defined bytes only
            out = ref_reduce(img[r0:r0 + plan.slot(l)], w, h, plan.steps[l])
            r1 = plan.levels[l + 1][2]
            assert out.shape == plan.written(l + 1)[::-1]
            img[r1:r1 + out.shape[0], :out.shape[1]] = out
    return img, mask


@functools.lru_cache(maxsize=None)
def drawing(index):
    from pislam_amd import synth
    return synth.make_level0(index)                      # 640 x 480


def make_frames(W, H, B, seed):
    """Frame 0 random, frame 1 the synth.make_level0 drawing cropped, frame 2 random 0 / 255 (the extreme of every
    rounding), and so on in turn; no byte equals POISON."""
    rng = np.random.default_rng(seed)
    out = np.empty((B, H, W), np.uint8)
    for b in range(B):
        if b % 3 == 0:
            out[b] = rng.integers(0, 256, (H, W), dtype=np.uint8)
        elif b % 3 == 1:
            y0 = 37 * (b // 3) % 300
            out[b] = drawing(b // 3 % 3)[y0:y0 + H, 101:101 + W]
        else:
            out[b] = rng.integers(0, 2, (H, W), dtype=np.uint8) * 255
    out[out == POISON] = POISON + 1
    return out


@functools.lru_cache(maxsize=None)
def reference(case, vstep_add, blur, seed):
    """-> (frames [B][H][W], images [B][rows][vstep], mask [rows][vstep]) of a case, computed once"""
    W, H, steps, vmin, B = case
    plan = Plan(W, H, steps, vmin, vstep_add)
    frames = make_frames(W, H, B, seed)
    built = [ref_build(f, plan, blur) for f in frames]
    for a in (frames, built[0][1]):
        a.flags.writeable = False
    return frames, np.stack([b[0] for b in built]), built[0][1]


def test_ref_build_equals_the_oracle_in_sequence(orc):
    """The anchor: ref_build == the oracle's gaussian5x5, then bilinear7_8 / bilinear13_16 level by level on a zeroed
    stacked buffer (what include/pislam_hip.h promises), on every byte; ref_layout == pislam_pyramid_layout."""
    from pislam_amd import capi
    lib = capi.load()
    for k, (W, H, steps, vmin, add) in enumerate([(3, 3, (), 0, 0), (5, 4, (), 0, 0), (5, 4, (1,), 0, 0), (97, 40, (2, 1, 2), 128, 0),
                                                   (259, 34, (2, 1, 2), 0, 3), (131, 35, (2, 1), 0, 1), (128, 65, (1, 2, 1), 0, 0),
                                                   (48, 40, (2, 1, 2), 0, 0)]):
        plan = Plan(W, H, steps, vmin, add)
        lv, vs, rows = (capi.Level * plan.n)(), ctypes.c_int32(0), ctypes.c_int32(0)
        st = (ctypes.c_int32 * max(1, len(steps)))(*steps)
        assert lib.pislam_pyramid_layout(W, H, plan.n, st, vmin, lv, ctypes.byref(vs), ctypes.byref(rows)) == 0
        assert [(l.width, l.height, l.row0) for l in lv] == plan.levels and all(l.col0 == 0 for l in lv)
        assert (vs.value + add, rows.value) == (plan.vstep, plan.rows)
        for b, frame in enumerate(make_frames(W, H, 3, 100 + k)):
            for blur in (True, False):
                exp = np.zeros((plan.rows, plan.vstep), np.uint8)
                exp[:H, :W] = frame
                if blur:
                    orc.gaussian5x5(exp, W, H)
                for l, step in enumerate(steps):
                    w, h, r0 = plan.levels[l]
                    tmp = exp[r0:].copy()                       # out of place: level l -> level l + 1's slot
                    (orc.bilinear7_8 if step == 1 else orc.bilinear13_16)(tmp, w, h)
                    ow, oh = plan.written(l + 1)
                    r1 = plan.levels[l + 1][2]
                    exp[r1:r1 + oh, :ow] = tmp[:oh, :ow]
                img, mask = ref_build(frame, plan, blur)
                assert (img == exp).all(), (W, H, steps, b, blur, np.argwhere(img != exp)[:4])
                assert (exp[~mask] == 0).all() and mask[:H, :W].all()


# ---- 3. the path rules, restated ---------------------------------------------------------------------------------------
# Addresses are byte offsets into an allocation whose base is 16-byte aligned (the harness asserts that of torch's).
def quad_kernel(src, dst, vstep, stride, nbx, N):
    """pp::k_bilinear4 runs (else the one-lane pp::k_bilinear): 16-byte loads of four blocks at once, dword stores."""
    return src % 16 == 0 and dst % 4 == 0 and vstep % 16 == 0 and stride % 16 == 0 and cdiv(nbx, 4) * 4 * N <= vstep


def reduction_kernels(plan, pyr_off, pstride):
    """Per reduction of a build: (step, nbx, 'quad' | 'generic')"""
    out = []
    for l, step in enumerate(plan.steps):
        N, _ = block(step)
        nbx = cdiv(plan.levels[l][0], N)
        q = quad_kernel(pyr_off + plan.levels[l][2] * plan.vstep, pyr_off + plan.levels[l + 1][2] * plan.vstep, plan.vstep, pstride, nbx, N)
        out.append((step, nbx, "quad" if q else "generic"))
    return out


def chain_eligible(plan, pyr_off, pstride):
    """The one-launch chain may run (option "build_chain"): three levels, the 4-block kernel on every reduction."""
    return plan.n >= 3 and all(k == "quad" for _, _, k in reduction_kernels(plan, pyr_off, pstride))


def gaussian_paths(W, frame_addr, frame_vstep):
    """Staging paths of one frame's tiles (128 columns each)."""
    paths = set()
    for x0 in range(0, W, 128):
        if frame_addr % 16 == 0 and frame_vstep % 16 == 0 and x0 + 128 <= W:
            paths.add("vector")
        elif frame_addr % 4 == 0 and frame_vstep % 4 == 0:
            paths.add("dword")
        else:
            paths.add("byte")
    return paths


def level0_stores(W, H, row_addr0, vstep):
    """How level 0's groups of four pixels are stored: as a dword, or bytewise at the right edge or at a misaligned row."""
    kinds = set()
    for y in range(H):
        if (row_addr0 + y * vstep) % 4:
            kinds.add("byte-misaligned")
        else:
            kinds.add("dword" if W >= 4 else "byte-edge")
            if W % 4:
                kinds.add("byte-edge")
    return kinds


def frame_layout(W, H, fl):
    off, pad, gap = fl
    return off, W + pad, H * (W + pad) + gap


def pyramid_layout(plan, pl):
    off, _, gap = pl
    return off, plan.rows * plan.vstep + gap


# ---- 4. the case matrix ------------------------------------------------------------------------------------------------
# (width, height, steps, vstep_min, batch)
SHAPES = [(3, 3, (), 0, 3), (5, 3, (), 0, 3),            # both reflections inside one dword; level 0 only
          (128, 65, (1, 2, 1), 0, 3),                    # one full vector tile, three tile rows (the last of 1 row); nbx 16, 7, 12
          (131, 35, (2, 1), 0, 3),                       # halo dword partly inside; level 0 generic, level 1 4-block: a mixed build
          (132, 33, (1, 2), 256, 3),                     # halo dword wholly inside; next tile 4 columns wide
          (259, 34, (2, 1, 2), 0, 3), (259, 34, (2, 1, 2), 320, 3),     # three tiles across; at 320 all 4-block, chain-eligible
          (80, 35, (2, 1), 128, 3),                      # nbx 5 (13/16), 9 (7/8)
          (100, 24, (1, 2), 128, 3),                     # nbx 13 (7/8), 6 (13/16)
          (104, 24, (2, 1), 128, 3),                     # nbx 7 (13/16), 11 (7/8)
          (97, 40, (2, 1, 2), 128, 9),                   # nbx 7, 10, 5; chain-eligible, batch 9
          (48, 40, (2, 1, 2), 0, 3)]                     # generic on every level
FRAME_LAYOUTS = [(0, 16, 0), (0, 4, 4), (0, 5, 0), (4, 0, 0), (1, 0, 0), (0, 16, 1), (3, 7, 9)]       # (off, pad, gap)
PYRAMID_LAYOUTS = [(0, 0, 16), (0, 0, 2), (0, 0, 1), (4, 0, 0), (1, 0, 0), (0, 4, 0), (0, 1, 0), (5, 3, 7)]   # (off, vstep_add, gap)


def matrix():
    """-> [(shape index, frame layout, pyramid layout, blur, margins_clean)]: every shape plain, then the layouts in pairs,
    dealt round the shapes; a few pairs are named because the coverage assertion asks for them."""
    runs = []
    for k in range(len(SHAPES)):
        runs.append((k, PLAIN, PLAIN, True, False))
        for t in range(3):
            runs.append((k, FRAME_LAYOUTS[(2 * k + 3 * t) % 7], PYRAMID_LAYOUTS[(3 * k + 3 * t + 1) % 8], True, False))
    runs += [(2, (0, 16, 0), PLAIN, True, False),        # 128x65: the vector path on padded rows, 4-block kernels behind it
             (2, (0, 16, 1), (0, 0, 16), True, False),   # frames 0, 1, 2 differ in alignment: vector and byte in one launch; chain, gap
             (10, (0, 4, 4), (0, 0, 16), True, False),   # the chain at batch 9 with a gap between pyramids
             (6, (4, 0, 0), (0, 0, 16), True, False),
             (3, (3, 7, 9), (0, 0, 2), False, False),    # no blur: hipMemcpy2DAsync from padded, gapped frames
             (7, (0, 4, 4), (5, 3, 7), True, True)]      # margins_clean on a buffer a plain build of the same layout filled
    return runs


def runs_of(k):
    return [r for r in matrix() if r[0] == k]


def test_matrix_covers_every_path():
    """From the restated rules alone: the matrix reaches every path the kernels choose between."""
    gauss, in_one_launch, quad, generic, mixed, chain, stores, margins_off16 = set(), set(), set(), set(), False, False, set(), False
    met_f, met_p = {}, {}
    for k, fl, pl, blur, clean in matrix():
        W, H, steps, vmin, B = SHAPES[k]
        plan = Plan(W, H, steps, vmin, pl[1])
        foff, fvstep, fstride = frame_layout(W, H, fl)
        poff, pstride = pyramid_layout(plan, pl)
        met_f.setdefault(fl, set()).add(k)
        met_p.setdefault(pl, set()).add(k)
        if blur:
            per_frame = [frozenset(gaussian_paths(W, foff + b * fstride, fvstep)) for b in range(B)]
            gauss |= set().union(*per_frame)
            if len(set().union(*per_frame)) > 1 and len(set(per_frame)) > 1:
                in_one_launch.add(frozenset(set().union(*per_frame)))
            for b in range(B):
                stores |= level0_stores(W, H, poff + b * pstride, plan.vstep)
        kernels = reduction_kernels(plan, poff, pstride)
        for step, nbx, kind in kernels:
            (quad if kind == "quad" else generic).add((step, nbx % 4))
        mixed |= len({kind for _, _, kind in kernels}) == 2
        chain |= chain_eligible(plan, poff, pstride) and B % 8 != 0 and pl[2] != 0
        margins_off16 |= not clean and poff % 16 != 0
    assert gauss == {"vector", "dword", "byte"}, gauss
    assert in_one_launch, "no launch whose frames take different Gaussian staging paths"
    assert quad == {(s, r) for s in (1, 2) for r in range(4)}, sorted(quad)
    assert {(s, r) for s in (1, 2) for r in (1, 2, 3)} <= generic, sorted(generic)      # output width nbx * M, M odd: no multiple of 4
    assert mixed and chain and margins_off16
    assert stores == {"dword", "byte-edge", "byte-misaligned"}, stores
    for fl in FRAME_LAYOUTS:
        assert len(met_f[fl]) >= 3, (fl, met_f[fl])
    for pl in PYRAMID_LAYOUTS:
        assert len(met_p[pl]) >= 3, (pl, met_p[pl])
    assert all(len(runs_of(k)) >= 4 for k in range(len(SHAPES)))
    # what the table of shapes promises
    assert [k for _, _, k in reduction_kernels(Plan(131, 35, (2, 1)), 0, Plan(131, 35, (2, 1)).rows * 144)] == ["generic", "quad"]
    assert chain_eligible(Plan(259, 34, (2, 1, 2), 320), 0, 16) and not chain_eligible(Plan(259, 34, (2, 1, 2)), 0, 16)
    assert chain_eligible(Plan(97, 40, (2, 1, 2), 128), 0, 16) and chain_eligible(Plan(128, 65, (1, 2, 1)), 0, 16)
    assert all(k == "generic" for _, _, k in reduction_kernels(Plan(48, 40, (2, 1, 2)), 0, 16))


# ---- 2. the layout harness -----------------------------------------------------------------------------------------------
def lay_frames(frames, fl):
    """-> (host buffer, frame_vstep, frame_stride): whole rows plus the gap for every frame, POISON wherever no pixel is"""
    B, H, W = frames.shape
    off, vs, stride = frame_layout(W, H, fl)
    host = np.full(off + B * stride, POISON, np.uint8)
    np.lib.stride_tricks.as_strided(host[off:], (B, H, vs), (stride, vs, 1))[:, :, :W] = frames
    return host, vs, stride


def lay_expected(plan, images, mask, pl, fill=SENT):
    """-> host buffer of the whole destination allocation: defined bytes from `images`, `fill` everywhere else"""
    B = images.shape[0]
    off, stride = pyramid_layout(plan, pl)
    host = np.full(off + B * stride, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(host[off:], (B, plan.rows, plan.vstep), (stride, plan.vstep, 1))
    view[:] = np.where(mask[None], images, view)
    return host


class Layouts:
    """Flat device buffers around a pyramid build: frames laid out by (off, pad, gap), pyramids by (off, vstep_add, gap)."""

    def __init__(self, ctx):
        import torch
        from pislam_amd import capi
        self.torch, self.ctx, self.lib, self.capi = torch, ctx, ctx.lib, capi

    def upload(self, host):
        t = self.torch.from_numpy(host if host.flags.writeable else host.copy()).cuda()
        assert t.data_ptr() % 16 == 0                       # the path rules count addresses from an aligned base
        return t

    def filled(self, n, value):
        t = self.torch.full((n,), value, dtype=self.torch.uint8, device="cuda")
        assert t.data_ptr() % 16 == 0
        return t

    def call(self, plan, frames_ptr, frame_vstep, frame_stride, batch, pyramids_ptr, pyramid_stride, flags):
        steps = (ctypes.c_int32 * max(1, len(plan.steps)))(*plan.steps)
        levels = (self.capi.Level * plan.n)(*[self.capi.Level(w, h, r0, 0) for w, h, r0 in plan.levels])
        return self.lib.pislam_pyramid_build_batch(self.ctx.h, plan.n, steps, levels, frames_ptr, frame_vstep, frame_stride, batch,
                                                   pyramids_ptr, plan.vstep, plan.rows, pyramid_stride, flags)

    def build(self, plan, frames, fl, dst, pl, flags):
        """One build of `frames` (host [B][H][W]) into the device buffer `dst`; returns once it has run."""
        src, fvstep, fstride = lay_frames(frames, fl)
        d_src = self.upload(src)
        poff, pstride = pyramid_layout(plan, pl)
        rc = self.call(plan, d_src.data_ptr() + fl[0], fvstep, fstride, frames.shape[0], dst.data_ptr() + poff, pstride, flags)
        assert rc == 0, self.lib.pislam_last_error(self.ctx.h)
        self.ctx.synchronize()

    def same(self, got, want, what):
        got = got.cpu().numpy()
        assert got.shape == want.shape
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[:6]}: got {got[bad[:6]]} want {want[bad[:6]]}"

    def chain_settings(self, plan, pl):
        """Both settings of "build_chain" where the rules let the chain run, else the default alone."""
        return (1, 0) if chain_eligible(plan, *pyramid_layout(plan, pl)) else (0,)

    def run(self, k, fl, pl, blur=True, clean=False):
        case = SHAPES[k]
        W, H, steps, vmin, B = case
        plan = Plan(W, H, steps, vmin, pl[1])
        frames, images, mask = reference(case, pl[1], blur, 1000 + k)
        want = lay_expected(plan, images, mask, pl)
        for chain in self.chain_settings(plan, pl):
            tag = f"{case} frames {fl} pyramids {pl} blur={blur} clean={clean} chain={chain}"
            dst = self.filled(want.size, SENT)
            self.ctx.set_option("build_chain", chain)
            try:
                if clean:                                   # other frames first: a plain build of the same layout
                    self.build(plan, reference(case, pl[1], blur, 2000 + k)[0], fl, dst, pl, BLUR if blur else 0)
                self.build(plan, frames, fl, dst, pl, (BLUR if blur else 0) | (CLEAN if clean else 0))
            finally:
                self.ctx.set_option("build_chain", 0)
            self.same(dst, want, tag)


@pytest.fixture(scope="module")
def lay(gpu_ctx):
    return Layouts(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["%dx%d-%s-%d" % (s[0], s[1], "".join(map(str, s[2])) or "0", s[3]) for s in SHAPES])
def test_gpu_matrix_against_ref_build(lay, k):
    """Every run of the matrix for one shape: the whole destination allocation against ref_build, bit for bit."""
    for _, fl, pl, blur, clean in runs_of(k):
        lay.run(k, fl, pl, blur, clean)


# ---- 5. the margins check on a misaligned layout -------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_check_margins_sees_exactly_the_margins(lay):
    """PISLAM_BUILD_CHECK_MARGINS at pyramids 5 bytes off, vstep + 3, 7 bytes apart: clean after a plain build, dirty with
    the one margin byte farthest from the origin set, clean again with the first byte beyond it set instead."""
    k, fl, pl = 7, (3, 7, 9), (5, 3, 7)
    case = SHAPES[k]
    W, H, steps, vmin, B = case
    plan = Plan(W, H, steps, vmin, pl[1])
    frames, images, mask = reference(case, pl[1], True, 1000 + k)
    poff, pstride = pyramid_layout(plan, pl)
    dst = lay.filled(poff + B * pstride, SENT)
    lay.build(plan, frames, fl, dst, pl, BLUR)
    lay.build(plan, frames, fl, dst, pl, BLUR | CLEAN | CHECK)
    cols, rows = plan.margin(plan.n - 1)
    assert cols < plan.vstep                                 # the byte to the right of the margin is in the same row
    last = poff + (B - 1) * pstride + (plan.levels[-1][2] + rows - 1) * plan.vstep + cols - 1
    assert mask[plan.levels[-1][2] + rows - 1, cols - 1] and not mask[plan.levels[-1][2] + rows - 1, cols]
    src, fvstep, fstride = lay_frames(frames, fl)
    d_src = lay.upload(src)

    def check():
        rc = lay.call(plan, d_src.data_ptr() + fl[0], fvstep, fstride, B, dst.data_ptr() + poff, pstride, BLUR | CLEAN | CHECK)
        lay.ctx.synchronize()
        return rc

    assert int(dst[last]) == 0
    dst[last] = 1
    assert check() == INVALID and b"margins" in lay.lib.pislam_last_error(lay.ctx.h)
    dst[last] = 0
    dst[last + 1] = 1
    assert check() == 0, lay.lib.pislam_last_error(lay.ctx.h)
    want = lay_expected(plan, images, mask, pl)
    want[last + 1] = 1
    lay.same(dst, want, "after the checks")


# ---- 6. limits -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case,chain", [((8, 8, (1,), 0, 65537), 0), ((64, 16, (2, 1), 0, 65537), 1)], ids=["8x8-generic", "64x16-chain"])
def test_gpu_batch_past_65535(lay, case, chain):
    """65537 frames.  The build puts the batch into grid.z (Gaussian, both reduction kernels) and grid.y (margins) as it is:
    HIP on gfx950 launches such a grid, and this test is what says so (include/pislam_hip.h).  Frame b is distinct frame
    b % 251 (the expectation is computed once per distinct frame), so frames 65535.. differ from frames 0.. at the index a
    16-bit grid coordinate would wrap to.  8 x 8 takes the one-lane kernel, 64 x 16 the one-launch chain (8193 groups of
    eight frames).  The whole destination is compared on the device."""
    torch = lay.torch
    W, H, steps, vmin, B = case
    plan = Plan(W, H, steps, vmin)
    assert chain_eligible(plan, 0, plan.rows * plan.vstep) == bool(chain)
    assert [k for _, _, k in reduction_kernels(plan, 0, plan.rows * plan.vstep)] == (["quad", "quad"] if chain else ["generic"])
    distinct = make_frames(W, H, 251, 60)
    built = [ref_build(f, plan) for f in distinct]
    want = np.stack([np.where(m, img, SENT) for img, m in built]).reshape(251, -1)
    pick = torch.arange(B, device="cuda") % 251
    frames = lay.upload(distinct)[pick].contiguous()
    dst = lay.filled(B * plan.rows * plan.vstep, SENT)
    lay.ctx.set_option("build_chain", chain)
    try:
        rc = lay.call(plan, frames.data_ptr(), W, H * W, B, dst.data_ptr(), plan.rows * plan.vstep, BLUR)
        assert rc == 0, lay.lib.pislam_last_error(lay.ctx.h)
        lay.ctx.synchronize()
    finally:
        lay.ctx.set_option("build_chain", 0)
    ok = (dst.view(B, -1) == lay.upload(want)[pick]).all(dim=1)
    bad = torch.nonzero(~ok).reshape(-1)
    assert bad.numel() == 0, f"{bad.numel()} pyramids differ, first {bad[:8].tolist()}"


@pytest.mark.gpu
def test_gpu_strides_past_4_gib(lay):
    """Two frames whose strides put the second one beyond 4 GiB: pyramid_stride 2^32 + 16 (the chain) and 2^32 + 1 (misaligned
    for the second pyramid: the one-lane kernels), then frame_stride 2^32 + 1.  Each buffer is one allocation, as in
    test_clahe.py; only the pyramids, a guard band of the sentinel around each and the frames' own bytes are set and
    looked at — the band behind pyramid 0 is the beginning of the region between the two."""
    torch = lay.torch
    case, G = SHAPES[10][:4] + (2,), 4096
    W, H, steps, vmin, B = case
    plan = Plan(W, H, steps, vmin)
    frames, images, mask = reference(case, 0, True, 70)
    size = plan.rows * plan.vstep
    big = (1 << 32) + 16
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * (big + size + 2 * G) + (1 << 30):
        pytest.skip("two buffers of 4 GiB do not fit the free device memory")
    one = np.full((B, G + size + G), SENT, np.uint8)
    one[:, G:G + size] = np.where(mask[None], images, SENT).reshape(B, -1)
    dst = src = None
    try:
        dst = torch.empty((G + big + size + G,), dtype=torch.uint8, device="cuda")
        assert dst.data_ptr() % 16 == 0
        d_frames = lay.upload(frames)
        for pstride, chain in ((big, 1), ((1 << 32) + 1, 0)):
            assert chain_eligible(plan, G, pstride) == bool(chain)
            for b in range(B):
                dst[b * pstride:b * pstride + G + size + G] = SENT
            lay.ctx.set_option("build_chain", chain)
            try:
                rc = lay.call(plan, d_frames.data_ptr(), W, H * W, B, dst.data_ptr() + G, pstride, BLUR)
                assert rc == 0, lay.lib.pislam_last_error(lay.ctx.h)
                lay.ctx.synchronize()
            finally:
                lay.ctx.set_option("build_chain", 0)
            for b in range(B):
                lay.same(dst[b * pstride:b * pstride + G + size + G], one[b], f"pyramid_stride {pstride}, pyramid {b}")
        fstride = (1 << 32) + 1
        src = torch.empty((G + fstride + H * W + G,), dtype=torch.uint8, device="cuda")
        for b in range(B):
            src[b * fstride:b * fstride + G + H * W + G] = POISON
            src[G + b * fstride:G + b * fstride + H * W] = d_frames[b].reshape(-1)
        small = lay.filled(B * size, SENT)
        rc = lay.call(plan, src.data_ptr() + G, W, fstride, B, small.data_ptr(), size, BLUR)
        assert rc == 0, lay.lib.pislam_last_error(lay.ctx.h)
        lay.ctx.synchronize()
        lay.same(small, lay_expected(plan, images, mask, PLAIN), f"frame_stride {fstride}")
    finally:
        dst = src = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---- 7. hipGraph replay --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_chain_build_replays_from_a_hipgraph(gpu_ctx):
    """The one-launch chain re-arms its own counters: one build with margins_clean captured on a side stream of a context
    of its own, replayed three times with new frames in the same frame buffer, every result against the reference of the
    frames it should have read; an eager build afterwards too."""
    import torch
    from pislam_amd.capi import Context
    k, fl, pl = 10, (0, 16, 0), (0, 0, 16)
    case = SHAPES[k]
    W, H, steps, vmin, B = case
    plan = Plan(W, H, steps, vmin)
    assert chain_eligible(plan, *pyramid_layout(plan, pl)) and B % 8
    poff, pstride = pyramid_layout(plan, pl)
    side = torch.cuda.Stream(torch.device("cuda:0"))
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        ctx.set_option("build_chain", 1)
        own = Layouts(ctx)
        host, fvstep, fstride = lay_frames(reference(case, 0, True, 3000)[0], fl)
        src = own.upload(host)
        dst = own.filled(poff + B * pstride, SENT)

        def build(flags):
            rc = own.call(plan, src.data_ptr() + fl[0], fvstep, fstride, B, dst.data_ptr() + poff, pstride, flags)
            assert rc == 0, own.lib.pislam_last_error(ctx.h)

        build(BLUR)                                          # sizes the counters and establishes the margins
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            build(BLUR | CLEAN)
        for seed in (3001, 3002, 3003, 3004):
            frames, images, mask = reference(case, 0, True, seed)
            src.copy_(torch.from_numpy(lay_frames(frames, fl)[0]).cuda())
            if seed < 3004:
                g.replay()
            else:
                build(BLUR | CLEAN)
            side.synchronize()
            ctx.synchronize()
            own.same(dst, lay_expected(plan, images, mask, pl), f"replay with frames {seed}")
        ctx.close()


# ---- 8. the stand-alone calls at device pointers ---------------------------------------------------------------------------
TAIL = 37                                                # bytes behind the last row, part of both allocations


def standalone_vsteps(kind, w):
    return (144, 145) if kind == 0 and w > 64 else (64, 65, 68)


def standalone_cases(kind):
    """-> [(w, h, vstep, off, in_place)]; kind 0 = gaussian5x5, 1 = bilinear7_8, 2 = bilinear13_16"""
    ws, hs = ((3, 4, 5, 16, 63, 129, 132), (3, 31, 33)) if kind == 0 else ((1, 7, 8, 9, 25, 33, 47), (1, 8, 17, 47))
    return [(w, h, vs, off, ip) for w in ws for h in hs for vs in standalone_vsteps(kind, w) for off in (0, 1, 4) for ip in (False, True)]


def standalone_kernel(kind, w, vstep, off, in_place):
    """The rule of part 3 for one stand-alone reduction.  In place the library reads from a private copy of the source in
    its own (aligned) workspace and writes to the caller's buffer."""
    N, _ = block(kind)
    return "quad" if quad_kernel(0 if in_place else off, off, vstep, 0, cdiv(w, N), N) else "generic"


def test_standalone_cases_reach_the_generic_kernel():
    """Every offset and every vstep that is no multiple of 16 sends an out-of-place reduction to the one-lane kernel; the
    aligned cases keep the 4-block kernel in the comparison."""
    for kind in (1, 2):
        kernels = {c: standalone_kernel(kind, c[0], c[2], c[3], c[4]) for c in standalone_cases(kind)}
        for (w, h, vs, off, ip), kernel in kernels.items():
            if not ip and (off or vs % 16):
                assert kernel == "generic"
            if off == 0 and vs == 64:
                assert kernel == "quad"
        assert {(c[0], c[1]) for c, kernel in kernels.items() if kernel == "generic"} == {(c[0], c[1]) for c in kernels}
    paths = set()
    for w, _, vs, off, in_place in standalone_cases(0):
        if not in_place:
            paths |= gaussian_paths(w, off, vs)
    assert paths == {"vector", "dword", "byte"}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["gaussian5x5", "bilinear7_8", "bilinear13_16"])
def test_gpu_standalone_calls_at_device_pointers(lay, kind):
    """Device-resident source and destination at base offsets 0, 1, 4 and rows of 64, 65, 68 (144, 145) bytes, out of place
    and in place: the whole destination allocation against the reference.  The reductions' block padding holds random
    bytes (the reference reads them too); what lies beyond it holds POISON."""
    from pislam_amd import synth
    torch = lay.torch
    fn = (lay.lib.pislam_gaussian5x5, lay.lib.pislam_bilinear7_8, lay.lib.pislam_bilinear13_16)[kind]
    N, M = (1, 1) if kind == 0 else block(kind)
    rng = np.random.default_rng(80 + kind)
    content, expect = {}, {}
    for w, h, vstep, off, in_place in standalone_cases(kind):
        wpad, hpad = cdiv(w, N) * N, cdiv(h, N) * N
        key = (w, h, vstep)
        if key not in content:
            a = rng.integers(0, 256, (hpad, vstep), dtype=np.uint8)
            a[a == POISON] = POISON + 1
            a[:, wpad:] = POISON
            content[key] = a
            expect[key] = synth.gaussian5x5(a[:h, :w]) if kind == 0 else ref_reduce(a, w, h, kind)
        a, out = content[key], expect[key]
        oh, ow = out.shape
        host = np.full(off + hpad * vstep + TAIL, POISON, np.uint8)
        host[off:off + hpad * vstep] = a.reshape(-1)
        src = lay.upload(host)
        if in_place:
            dst, want = src, host.copy()
        else:
            want = np.full(off + hpad * vstep + TAIL, SENT, np.uint8)
            dst = lay.filled(want.size, SENT)
        np.lib.stride_tricks.as_strided(want[off:], (oh, ow), (vstep, 1))[:] = out
        rc = fn(lay.ctx.h, vstep, w, h, src.data_ptr() + off, dst.data_ptr() + off)
        assert rc == 0, lay.lib.pislam_last_error(lay.ctx.h)
        lay.ctx.synchronize()
        lay.same(dst, want, f"kind {kind} {w}x{h} vstep {vstep} off {off} in_place={in_place}")
        if not in_place:
            lay.same(src, host, "the source")
