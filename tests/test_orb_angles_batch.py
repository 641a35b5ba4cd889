"""Batched rotation bins (pislam_orb_angles_batch): the angle orbCompute rotates its pattern by,
for every keypoint of a batch of pyramids.

The expectation is the oracle's: `orc.atan2_bins(orc.orb_centroids(img, kp))` — the reference's own moments and bin.
The GPU tests pre-fill the output with the sentinel byte and compare bit for bit.  The grid, launch, coordinate and
address limits are in test_after_match_limits.py."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_match_window import COUNT_INVALID, SENTINEL, clamp_count

S8 = SENTINEL & 0xFF


def ref_angles(orc, img, kp):
    """uint8 [n]: the oracle's bin per keypoint; 0xff where the 31 x 31 patch would leave img (nothing is read there)."""
    kp = np.asarray(kp, np.uint32)
    rows, vstep = img.shape
    x, y = (kp >> 12) & 0xFFF, kp & 0xFFF
    ok = (x >= 15) & (x <= vstep - 16) & (y >= 15) & (y <= rows - 16)
    out = np.full(len(kp), 0xFF, np.uint8)
    if ok.any():
        good = np.ascontiguousarray(kp[ok])
        out[ok] = orc.atan2_bins(orc.orb_centroids(np.ascontiguousarray(img), good))[:len(good)]
    return out


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_header_binding_and_wrappers_declare_the_two_calls():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+pislam_orb_angles_batch\s*\(", code)
    assert re.search(r"\bint\s+pislam_match_select_batch\s*\(", code)
    m = re.search(r"typedef\s+struct\s+pislam_select_params\s*\{(.*?)\}\s*pislam_select_params\s*;", code, flags=re.S)
    assert m, "pislam_select_params is not declared"
    fields = re.findall(r"\b([a-z_0-9]+)\s*[,;]", m.group(1))
    assert fields == ["max_dist", "ratio_num", "ratio_den", "unique", "rot_keep", "rot_min_pct"]
    from pislam_amd import capi, frontend
    assert "pislam_orb_angles_batch" in capi.SYMBOLS and "pislam_match_select_batch" in capi.SYMBOLS
    assert [f[0] for f in capi.SelectParams._fields_] == fields
    assert callable(frontend.orbAnglesBatch) and callable(frontend.selectMatchesBatch)
    assert callable(frontend.OrbFrontend.angles)


# ---- GPU -------------------------------------------------------------------------------------------------------------
def run_angles(ctx, img, kp, counts):
    import torch
    from pislam_amd.frontend import orbAnglesBatch
    dev = torch.device("cuda:0")
    ang = torch.full(kp.shape, S8, dtype=torch.uint8, device=dev)
    orbAnglesBatch(torch.from_numpy(img).to(dev), torch.from_numpy(kp.view(np.int32)).to(dev),
                   torch.from_numpy(np.asarray(counts, np.uint32).view(np.int32)).to(dev), ang, ctx=ctx)
    torch.cuda.synchronize()
    return ang.cpu().numpy()


def check_angles(orc, got, img, kp, counts):
    for b in range(len(img)):
        n = clamp_count(counts[b], kp.shape[1])
        assert (got[b, :n] == ref_angles(orc, img[b], kp[b, :n])).all(), b
        assert (got[b, n:] == S8).all(), ("slot past the count written", b)


@pytest.mark.gpu
def test_gpu_angles_of_the_fixture_pyramids(gpu_ctx, orc, demo, synth_small):
    """The two golden pyramids as one batch (the small one in the top left corner of a buffer of the demo's shape), each
    with its own oracle keypoint list; then the same batch with an invalid count, a count above the stride and 0."""
    big = demo["img"]
    small = np.zeros_like(big)
    s = synth_small["img"]
    small[:s.shape[0], :s.shape[1]] = s
    k0, _, _ = orc.pyramid(big, demo["levels"])
    k1, _, _ = orc.pyramid(small, synth_small["levels"])
    assert len(k0) == len(demo["kp"]) and len(k1) == len(synth_small["kp"]) and len(k1) > 0
    stride = len(k0) + 5
    img = np.stack([big, small])
    kp = np.zeros((2, stride), np.uint32)
    kp[0, :len(k0)], kp[1, :len(k1)] = k0, k1
    counts = [len(k0), len(k1)]
    got = run_angles(gpu_ctx, img, kp, counts)
    check_angles(orc, got, img, kp, counts)
    assert set(got[0, :len(k0)].tolist()) == set(range(30))          # every bin occurs: no constant can pass
    assert (got[0, :len(k0)] == demo["angles"][:len(k0)]).all()      # and these are the recorded reference angles
    img5 = np.stack([big, small, big, big, small])
    kp5 = np.concatenate([kp, kp[0:1], kp[0:1], kp[1:2]])
    counts5 = counts + [COUNT_INVALID, stride + 1000, 0]
    got = run_angles(gpu_ctx, img5, kp5, counts5)
    check_angles(orc, got, img5, kp5, counts5)
    assert (got[2] == S8).all() and (got[4] == S8).all() and (got[3] != S8).any()


@pytest.mark.gpu
def test_gpu_angles_patch_limits(gpu_ctx, orc):
    """A 64 x 48 image: the four corners of the valid range equal the oracle, one step outside gives 0xff."""
    rng = np.random.default_rng(48)
    img = rng.integers(0, 256, (1, 48, 64), dtype=np.uint8)
    inside = [(15, 15), (48, 15), (15, 32), (48, 32), (30, 20)]
    outside = [(14, 15), (49, 15), (15, 14), (15, 33), (14, 14), (49, 33), (0, 0), (63, 47), (4095, 4095), (30, 4095)]
    pts = inside + outside
    kp = np.array([[(0xAB << 24) | (x << 12) | y for x, y in pts]], np.uint32)      # score bits are ignored
    got = run_angles(gpu_ctx, img, kp, [len(pts)])
    check_angles(orc, got, img, kp, [len(pts)])
    assert (got[0, :len(inside)] < 30).all() and (got[0, len(inside):] == 0xFF).all()


@pytest.mark.gpu
def test_gpu_angles_rejects_bad_arguments(gpu_ctx):
    import torch
    from pislam_amd.capi import ptr
    dev = torch.device("cuda:0")
    img = torch.zeros((2, 48, 64), dtype=torch.uint8, device=dev)
    kp = torch.full((2, 8), (20 << 12) | 20, dtype=torch.int32, device=dev)
    cnt = torch.full((2,), 8, dtype=torch.int32, device=dev)
    ang = torch.full((2, 8), S8, dtype=torch.uint8, device=dev)

    def call(img=img, kp=kp, cnt=cnt, ang=ang, vstep=64, rows=48, batch=2):
        rc = gpu_ctx.lib.pislam_orb_angles_batch(gpu_ctx.h, ptr(img), vstep, rows, 64 * 48, ptr(kp), ptr(cnt), 8, batch, ptr(ang))
        torch.cuda.synchronize()
        return rc

    for bad in (dict(img=img.cpu()), dict(kp=kp.cpu()), dict(cnt=cnt.cpu()), dict(ang=ang.cpu()), dict(img=None), dict(kp=None),
                dict(cnt=None), dict(ang=None), dict(batch=-1), dict(vstep=30), dict(rows=30)):
        assert call(**bad) == -1, list(bad)
        assert bool((ang == S8).all()), list(bad)
    assert call(batch=0) == 0 and bool((ang == S8).all())
    assert call() == 0 and bool((ang < 30).all())
