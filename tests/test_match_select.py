"""On-device match selection (pislam_match_select_batch): distance threshold, ratio test,
cross-check, one-to-one claim, ORB-SLAM's rotation histogram, compaction into pair lists.

The semantics are the library's own (include/pislam_hip.h).  `ref_select` states them independently of the library:
one boolean mask per test applied in order, a minimum of dist << 32 | i per train index for the claim, a bincount and
a sort by (-count, bin) for the histogram.  The CPU tests check that reference on hand-built cases and on the demo
photograph against its 180 degree rotation; the GPU tests compare the library with it bit for bit, outputs pre-filled
with a sentinel.  The block, chunk, index and batch limits are in test_after_match_limits.py."""
import ctypes

import numpy as np
import pytest

from test_match_window import COUNT_INVALID, NONE_U32, SENTINEL, clamp_count

S8 = SENTINEL & 0xFF
OFF = dict(max_dist=256, ratio=None, unique=0, rot_keep=0, rot_min_pct=0)
ORBSLAM = dict(max_dist=50, ratio=(8, 10), unique=1, rot_keep=3, rot_min_pct=10)


# ---- the reference ---------------------------------------------------------------------------------------------------
def ref_select(idx, dist, dist2, nt, *, max_dist=50, ratio=(8, 10), unique=1, rot_keep=3, rot_min_pct=10, back=None,
               qa=None, ta=None):
    """One pair, its nq queries: (sel_q int32, sel_t int32, status uint8 [nq], hist int64 [30])."""
    nq = len(idx)
    i = np.arange(nq, dtype=np.int64)
    j = np.asarray(idx, np.int32).astype(np.int64)
    d = np.asarray(dist).astype(np.uint32).astype(np.int64)
    status = np.zeros(nq, np.uint8)
    alive = np.ones(nq, bool)

    def fail(mask, code):
        m = alive & mask
        status[m] = code
        alive[m] = False

    fail((j < 0) | (j >= nt), 1)
    jj = np.where(alive, j, 0)                                       # (an index that is safe to gather with)
    fail(d > max_dist, 2)
    if ratio is not None and ratio[1] > 0:
        d2 = np.asarray(dist2).astype(np.uint32).astype(np.int64)
        fail((d2 != 0xFFFFFFFF) & (d * ratio[1] >= d2 * ratio[0]), 3)
    if back is not None and nt > 0:
        fail(np.asarray(back, np.int32).astype(np.int64)[jj] != i, 4)
    if unique:
        key = (d << 32) | i
        best = np.full(max(nt, 1), np.iinfo(np.int64).max, np.int64)
        np.minimum.at(best, jj[alive], key[alive])
        fail(key != best[jj], 5)
    hist = np.zeros(30, np.int64)
    if rot_keep > 0:
        a, t = np.asarray(qa, np.uint8).astype(np.int64), np.asarray(ta, np.uint8).astype(np.int64)[jj] if nt else i * 0
        fail((a >= 30) | (t >= 30), 6)
        bins = (a - t + 30) % 30
        hist = np.bincount(bins[alive], minlength=30).astype(np.int64)
        order = sorted(range(30), key=lambda k: (-int(hist[k]), k))
        rank = np.empty(30, np.int64)
        rank[order] = np.arange(30)
        top = int(hist[order[0]])
        keep = (rank < rot_keep) & (hist >= 1) & (100 * hist >= rot_min_pct * top)
        fail(~keep[np.where(alive, bins, 0)], 6)
    sel = np.flatnonzero(alive)
    return sel.astype(np.int32), j[sel].astype(np.int32), status, hist


def arr(v, dt=np.uint32):
    return np.asarray(v, dt)


# ---- CPU: the reference itself -----------------------------------------------------------------------------------
def test_reference_one_case_per_status_code():
    #        no match  too far  ratio  selected  loses the claim  wrong bin
    idx = arr([-1, 9, 0, 1, 2, 3, 4, 4, 5, 6, 7, 7], np.int32)
    dist = arr([NONE_U32, NONE_U32, 51, 40, 10, 20, 30, 31, 10, 10, 10, 10])
    dist2 = arr([NONE_U32, NONE_U32, 90, 50, 90, 90, 90, 90, 90, 90, 90, 90])
    qa = arr([0, 0, 0, 0, 3, 3, 3, 3, 3, 3, 7, 3], np.uint8)
    ta = arr([0] * 8, np.uint8)
    kw = dict(max_dist=50, ratio=(8, 10), unique=1, rot_keep=1, rot_min_pct=10, qa=qa, ta=ta)
    sq, st, status, hist = ref_select(idx, dist, dist2, 8, **kw)
    #  0: idx -1; 1: idx 9 >= nt; 2: 51 > 50; 3: 40 * 10 >= 50 * 8; 4, 5, 6, 8, 9: bin 3; 7: loses train 4 to query 6
    #  (30 < 31); 10: bin 7 is not the top bin; 11: loses train 7 to query 10 (equal distance, smaller index) although
    #  query 10 is then cut by the rotation test: the claim is decided among the survivors of tests 1-4
    assert status.tolist() == [1, 1, 2, 3, 0, 0, 0, 5, 0, 0, 6, 5]
    assert sq.tolist() == [4, 5, 6, 8, 9] and st.tolist() == [2, 3, 4, 5, 6]
    assert hist[3] == 5 and hist[7] == 1 and hist.sum() == 6
    # the cross-check: train 2's own best query is 9, so query 4 goes; a query the cross-check removes claims nothing
    # (query 7 fails it too: train 4 points back at 6)
    back = arr([2, 3, 9, 5, 6, 8, 9, 10], np.int32)
    sq, st, status, hist = ref_select(idx, dist, dist2, 8, back=back, **kw)
    assert status.tolist() == [1, 1, 2, 3, 4, 0, 0, 4, 0, 0, 6, 4] and sq.tolist() == [5, 6, 8, 9] and hist[3] == 4


def test_reference_claim_ties_and_distances():
    # two queries on one train with equal distance: the smaller i wins; a smaller distance beats a smaller index
    sq, st, status, _ = ref_select(arr([0, 0, 1, 1], np.int32), arr([7, 7, 9, 8]), None, 2, ratio=None, rot_keep=0)
    assert status.tolist() == [0, 5, 5, 0] and sq.tolist() == [0, 3] and st.tolist() == [0, 1]
    # without the switch both stay
    sq, _, status, _ = ref_select(arr([0, 0], np.int32), arr([7, 7]), None, 1, ratio=None, unique=0, rot_keep=0)
    assert sq.tolist() == [0, 1] and not status.any()


def test_reference_ratio_boundaries():
    idx = arr([0, 1, 2, 3], np.int32)
    dist = arr([40, 40, 39, 0])
    dist2 = arr([NONE_U32, 50, 50, 0])
    _, _, status, _ = ref_select(idx, dist, dist2, 4, ratio=(8, 10), unique=0, rot_keep=0)
    # no second candidate passes; 40 * 10 == 50 * 8 fails; 39 * 10 < 400 passes; 0 * 10 >= 0 * 8 fails
    assert status.tolist() == [0, 3, 0, 3]


def test_reference_histogram_ties_and_percentage():
    # two bins of equal count with rot_keep 1: the smaller bin is kept
    qa = arr([4, 4, 9, 9], np.uint8)
    kw = dict(max_dist=256, ratio=None, unique=0)
    sq, _, status, hist = ref_select(arr([0, 1, 2, 3], np.int32), arr([1] * 4), None, 4, rot_keep=1, rot_min_pct=0, qa=qa,
                                     ta=arr([0] * 4, np.uint8), **kw)
    assert hist[4] == 2 and hist[9] == 2 and sq.tolist() == [0, 1] and status.tolist() == [0, 0, 6, 6]
    # top bin 100, rot_min_pct 10: a bin of 10 is kept, a bin of 9 is dropped
    qa = arr([5] * 100 + [6] * 10 + [7] * 9, np.uint8)
    n = len(qa)
    sq, _, status, hist = ref_select(np.arange(n, dtype=np.int32), arr([1] * n), None, n, rot_keep=3, rot_min_pct=10, qa=qa,
                                     ta=arr([0] * n, np.uint8), **kw)
    assert (hist[5], hist[6], hist[7]) == (100, 10, 9)
    assert (status[:110] == 0).all() and (status[110:] == 6).all() and len(sq) == 110
    # the difference wraps: query bin 2 against train bin 29 is bin 3
    _, _, _, hist = ref_select(arr([0], np.int32), arr([1]), None, 1, rot_keep=1, rot_min_pct=0, qa=arr([2], np.uint8),
                               ta=arr([29], np.uint8), **kw)
    assert hist[3] == 1 and hist.sum() == 1


def test_reference_invalid_angle_is_not_counted():
    qa = arr([0xFF, 3, 3], np.uint8)
    ta = arr([0, 0xFF, 0], np.uint8)
    sq, _, status, hist = ref_select(arr([0, 1, 2], np.int32), arr([1] * 3), None, 3, max_dist=256, ratio=None, unique=0,
                                     rot_keep=30, rot_min_pct=0, qa=qa, ta=ta)
    assert status.tolist() == [6, 6, 0] and hist.sum() == 1 and hist[3] == 1 and sq.tolist() == [2]


def test_reference_all_off_selects_exactly_the_valid_idx():
    rng = np.random.default_rng(1)
    idx = rng.integers(-2, 12, 200).astype(np.int32)
    dist = rng.integers(0, 257, 200).astype(np.uint32)
    sq, st, status, hist = ref_select(idx, dist, None, 10, **OFF)
    valid = np.flatnonzero((idx >= 0) & (idx < 10))
    assert (sq == valid).all() and (st == idx[valid]).all() and not hist.any()
    assert (status[valid] == 0).all() and (np.delete(status, valid) == 1).all()


def rotated_photograph(demo):
    img = np.ascontiguousarray(demo["img"][:480, :640])
    return np.stack([img, np.ascontiguousarray(img[::-1, ::-1])])


def oracle_angles(orc, img, kp):
    return orc.atan2_bins(orc.orb_centroids(img, kp))[:len(kp)]


def test_reference_on_the_rotated_photograph(orc, demo):
    """Level 0 of the demo photograph against its 180 degree rotation, everything from the oracle: the rotation
    histogram peaks at bin 15 = 180 / 12 and only that bin survives ORB-SLAM's settings."""
    imgs = rotated_photograph(demo)
    lv = [(640, 480, 0)]
    kq, dq, _ = orc.pyramid(imgs[0], lv)
    kt, dt, _ = orc.pyramid(imgs[1], lv)
    assert (len(kq), len(kt)) == (271, 286)
    idx, dist, dist2 = orc.match_hamming(dq, dt)
    qa, ta = oracle_angles(orc, imgs[0], kq), oracle_angles(orc, imgs[1], kt)
    _, _, st4, _ = ref_select(idx, dist, dist2, len(kt), max_dist=50, ratio=(8, 10), unique=0, rot_keep=0)
    assert int((st4 == 0).sum()) == 168
    sq, st, status, hist = ref_select(idx, dist, dist2, len(kt), qa=qa, ta=ta, **ORBSLAM)
    assert int(hist.sum()) == 166 and int(hist.argmax()) == 15
    assert (int(hist[15]), int(hist[14]), int(hist[16])) == (157, 2, 7)
    assert len(sq) == 157 and ((qa[sq].astype(int) - ta[st].astype(int)) % 30 == 15).all()
    assert sorted(set(status.tolist())) == [0, 2, 3, 5, 6]


# ---- GPU -----------------------------------------------------------------------------------------------------------
def T(a, dev="cuda:0"):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(dev)


def run_select(ctx, case, want_status=True, want_hist=True, **params):
    """case: dict of numpy arrays idx, dist, dist2 (or None), qc, tc, ts, back / qa / ta (or None).  Outputs pre-filled
    with the sentinel; returns them as numpy (sel_q, sel_t, nsel, status or None, rot_hist or None)."""
    import torch
    from pislam_amd.frontend import selectMatchesBatch
    B, qs = case["idx"].shape
    dev = torch.device("cuda:0")
    full = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=dev)
    s32 = SENTINEL
    outs = dict(sel_q=full((B, qs), torch.int32, s32), sel_t=full((B, qs), torch.int32, s32), nsel=full((B,), torch.int32, s32),
                status=full((B, qs), torch.uint8, S8) if want_status else None,
                rot_hist=full((B, 30), torch.int32, s32) if want_hist else None)
    opt = lambda k: None if case.get(k) is None else T(case[k])
    selectMatchesBatch(T(case["idx"]), T(case["dist"]), opt("dist2"), T(case["qc"]), T(case["tc"]), back_idx=opt("back"),
                       qangle=opt("qa"), tangle=opt("ta"), t_stride=case["ts"], ctx=ctx, **params, **outs)
    torch.cuda.synchronize()
    np_ = lambda t: None if t is None else t.cpu().numpy()
    return tuple(np_(outs[k]) for k in ("sel_q", "sel_t", "nsel", "status", "rot_hist"))


def check_select(got, case, **params):
    sel_q, sel_t, nsel, status, rot_hist = got
    B, qs = case["idx"].shape
    s32 = SENTINEL
    row = lambda k, b, n: None if case.get(k) is None else case[k][b, :n]
    use_rot = params.get("rot_keep", 3) > 0 and case.get("qa") is not None
    for b in range(B):
        nq, nt = clamp_count(case["qc"][b], qs), clamp_count(case["tc"][b], case["ts"])
        kw = dict(params)
        if not use_rot:
            kw["rot_keep"] = 0
        eq, et, est, eh = ref_select(case["idx"][b, :nq], case["dist"][b, :nq], row("dist2", b, nq), nt, back=row("back", b, nt),
                                     qa=row("qa", b, nq) if use_rot else None, ta=row("ta", b, nt) if use_rot else None, **kw)
        n = int(nsel[b])
        assert n == len(eq), (b, params, n, len(eq))
        assert (sel_q[b, :n] == eq).all() and (sel_t[b, :n] == et).all(), (b, params)
        assert (sel_q[b, n:] == s32).all() and (sel_t[b, n:] == s32).all(), ("slot past nsel written", b, params)
        if status is not None:
            assert (status[b, :nq] == est).all(), (b, params, np.flatnonzero(status[b, :nq] != est)[:5])
            assert (status[b, nq:] == S8).all(), ("status past the query count written", b)
        if rot_hist is not None:
            assert (rot_hist[b] == eh).all(), (b, params, rot_hist[b], eh)


def random_case(rng, pairs, qs, ts):
    B = len(pairs)
    c = dict(ts=ts, idx=rng.integers(-1, 5, (B, qs)).astype(np.int32), dist=rng.integers(0, 257, (B, qs)).astype(np.uint32),
             dist2=np.zeros((B, qs), np.uint32), back=rng.integers(-1, qs, (B, ts)).astype(np.int32),
             qa=rng.choice(30, (B, qs), p=np.r_[[0.3, 0.2, 0.1], np.full(27, 0.4 / 27)]).astype(np.uint8),
             ta=rng.integers(0, 3, (B, ts)).astype(np.uint8),
             qc=arr([p[0] for p in pairs]), tc=arr([p[1] for p in pairs]))
    for b in range(B):
        nq, nt = clamp_count(c["qc"][b], qs), clamp_count(c["tc"][b], ts)
        c["idx"][b] = rng.integers(-1, nt + max(2, nt // 8), qs)            # some -1, some >= nt
        kind = rng.integers(0, 3, qs)                                      # dist2 below dist, above it, none
        d = c["dist"][b].astype(np.int64)
        c["dist2"][b] = np.where(kind == 0, d - rng.integers(0, 1 + d), np.where(kind == 1, d + rng.integers(0, 120, qs),
                                                                                 0xFFFFFFFF)).astype(np.uint32)
        ok = np.flatnonzero((c["idx"][b, :nq] >= 0) & (c["idx"][b, :nq] < nt))
        ok = ok[rng.random(len(ok)) < 0.5]                                  # about half consistent
        c["back"][b, c["idx"][b, ok]] = ok
    c["qa"][rng.random((B, qs)) < 0.02] = 0xFF
    c["ta"][rng.random((B, ts)) < 0.02] = 0xFF
    return c


def without(case, *keys):
    c = dict(case)
    for k in keys:
        c[k] = None
    return c


PAIRS = [(0, 5), (5, 0), (1, 1), (63, 64), (64, 65), (65, 63), (257, 3), (1000, 1000), (1000, 1), (1, 1000),
         (COUNT_INVALID, 9), (2000, 1500)]
GRID = [("off", OFF, ("back", "qa", "ta")),
        ("max_dist", dict(OFF, max_dist=50), ("back", "qa", "ta")),
        ("ratio", dict(OFF, ratio=(8, 10)), ("back", "qa", "ta")),
        ("back", OFF, ("qa", "ta")),
        ("unique", dict(OFF, unique=1), ("back", "qa", "ta")),
        ("rot", dict(OFF, rot_keep=3, rot_min_pct=10), ("back",)),
        ("orbslam", ORBSLAM, ("back",)),
        ("orbslam+back", ORBSLAM, ()),
        ("rot30", dict(OFF, unique=1, rot_keep=30, rot_min_pct=0), ("back",)),
        ("max_dist0", dict(ORBSLAM, max_dist=0), ("back",))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [g[0] for g in GRID])
def test_gpu_select_random(gpu_ctx, name):
    """12 pairs in one call, q_stride 1024 (the last pair's query count clamps); (257, 3) is the contended claim."""
    _, params, drop = next(g for g in GRID if g[0] == name)
    case = without(random_case(np.random.default_rng(5), PAIRS, 1024, 1500), *drop)
    got = run_select(gpu_ctx, case, **params)
    check_select(got, case, **params)
    assert int(got[2][7]) > 0 and int(got[2][0]) == 0 and int(got[2][10]) == 0
    if name == "orbslam":
        codes = set(got[3][7, :1000].tolist())
        assert codes == {0, 1, 2, 3, 5, 6}, codes


@pytest.mark.gpu
def test_gpu_select_chunk_limits(gpu_ctx):
    """t_stride 65535: the uniqueness table walks the train range in chunks of 16384.  Contested train indices on both
    sides of every chunk edge with differing and equal distances; a second pair whose second chunk has one slot."""
    rng = np.random.default_rng(16384)
    qs, ts = 300, 65535
    case = random_case(rng, [(300, 65535), (300, 16385)], qs, ts)
    case["dist"][:] = rng.integers(0, 60, (2, qs))
    hot = [16383, 16384, 32767, 32768, 49151, 49152, 65534]
    for k, j in enumerate(hot):                                    # six queries each: 3 distinct distances, 3 equal
        q = 10 + 6 * k + np.arange(6)
        case["idx"][0, q] = j
        case["dist"][0, q] = [9, 7, 8, 5, 5, 5] if k % 2 else [5, 5, 9, 5, 7, 8]
    case["idx"][1, :12] = [16384] * 6 + [16383] * 6
    case["dist"][1, :12] = [4, 3, 3, 9, 3, 8, 20, 20, 20, 1, 1, 30]
    case["dist2"][:, :64] = 0xFFFFFFFF
    for name, params, drop in (("unique", dict(OFF, unique=1), ("back", "qa", "ta")), ("orbslam", ORBSLAM, ("back",))):
        c = without(case, *drop)
        got = run_select(gpu_ctx, c, **params)
        check_select(got, c, **params)
        if name == "unique":
            st = got[3]
            assert st[0, 10:16].tolist() == [0, 5, 5, 5, 5, 5] and st[0, 16:22].tolist() == [5, 5, 5, 0, 5, 5]
            assert st[1, :12].tolist() == [5, 0, 5, 5, 5, 5, 5, 5, 5, 0, 5, 5]


@pytest.mark.gpu
def test_gpu_select_end_to_end_on_the_rotated_photograph(gpu_ctx, demo):
    """pislam_orb_frontend_batch -> pislam_match_hamming_batch -> pislam_orb_angles_batch -> pislam_match_select_batch
    on the photograph and its 180 degree rotation: every output equals the reference fed with the library's own matcher
    outputs and angles, and the histogram peaks at bin 15."""
    import torch
    from pislam_amd.frontend import OrbFrontend, matchHammingBatch
    dev = torch.device("cuda:0")
    pyr = torch.from_numpy(rotated_photograph(demo)).to(dev)
    fe = OrbFrontend([(640, 480, 0)], vstep=640, rows=480, max_keypoints=512, ctx=gpu_ctx)
    kp, desc, counts = fe.alloc_outputs(2, dev)
    fe(pyr, kp, desc, counts)
    idx, dist, dist2 = matchHammingBatch(desc[0:1], counts[0:1], desc[1:2], counts[1:2], ctx=gpu_ctx)
    ang = fe.angles(pyr, kp, counts)
    torch.cuda.synchronize()
    n = counts.cpu().numpy()
    assert n.tolist() == [271, 286]
    case = dict(idx=idx.cpu().numpy(), dist=dist.cpu().numpy().view(np.uint32), dist2=dist2.cpu().numpy().view(np.uint32),
                qc=n[0:1].view(np.uint32), tc=n[1:2].view(np.uint32), ts=512, qa=ang[0:1].cpu().numpy(), ta=ang[1:2].cpu().numpy())
    got = run_select(gpu_ctx, case, **ORBSLAM)
    check_select(got, case, **ORBSLAM)
    assert int(got[4][0].argmax()) == 15 and int(got[2][0]) == 157


@pytest.mark.gpu
def test_gpu_select_null_combinations(gpu_ctx):
    from pislam_amd.capi import PislamError
    case = random_case(np.random.default_rng(9), [(200, 150), (64, 64)], 256, 160)
    no_d2 = without(case, "dist2", "back")
    got = run_select(gpu_ctx, no_d2, **dict(ORBSLAM, ratio=None))                  # dist2 NULL, ratio off
    check_select(got, no_d2, **dict(ORBSLAM, ratio=None))
    no_ang = without(case, "qa", "ta")
    got = run_select(gpu_ctx, no_ang, **dict(ORBSLAM, rot_keep=0))                 # angles NULL, rotation off
    check_select(got, no_ang, **dict(ORBSLAM, rot_keep=0))
    assert not got[4].any()
    got = run_select(gpu_ctx, case, want_status=False, want_hist=False, **ORBSLAM)  # status NULL, rot_hist NULL
    check_select(got, case, **ORBSLAM)
    t = select_tensors(case)
    assert raw_select(gpu_ctx, t, ORBSLAM) == 0
    assert not bool((t["nsel"] == S8).all())
    t = select_tensors(case)                                                       # fresh sentinels for the refusals
    assert raw_select(gpu_ctx, t, ORBSLAM, dist2=None) == -1                       # a ratio without dist2
    assert raw_select(gpu_ctx, t, ORBSLAM, qangle=None, tangle=None) == -1         # a rotation check without angles
    assert raw_select(gpu_ctx, t, ORBSLAM, qangle=None) == -1
    assert raw_select(gpu_ctx, t, dict(ORBSLAM, rot_keep=0)) == -1                 # angles without a rotation check
    with pytest.raises(PislamError):
        run_select(gpu_ctx, no_d2, **ORBSLAM)
    assert_untouched(t)


OUT_KEYS = ("sel_q", "sel_t", "nsel", "status", "rot_hist")


def select_tensors(case):
    """Device tensors of a case under the C argument names, outputs pre-filled with the sentinel byte."""
    import torch
    B, qs = case["idx"].shape
    dev = torch.device("cuda:0")
    t = dict(idx=T(case["idx"]), dist=T(case["dist"]), dist2=T(case["dist2"]), qcounts=T(case["qc"]), tcounts=T(case["tc"]),
             back_idx=T(case["back"]), qangle=T(case["qa"]), tangle=T(case["ta"]), q_stride=qs, t_stride=case["ts"], batch=B)
    for k, shape in (("sel_q", (B, qs, 4)), ("sel_t", (B, qs, 4)), ("nsel", (B, 4)), ("status", (B, qs)), ("rot_hist", (B, 30, 4))):
        t[k] = torch.full(shape, S8, dtype=torch.uint8, device=dev)
    return t


def raw_select(ctx, t, params, **over):
    """The C call with some arguments replaced (None = NULL): the return code."""
    import torch
    from pislam_amd.capi import SelectParams, ptr
    a = dict(t)
    a.update(over)
    num, den = params["ratio"] or (0, 0)
    p = SelectParams(params["max_dist"], num, den, params["unique"], params["rot_keep"], params["rot_min_pct"])
    rc = ctx.lib.pislam_match_select_batch(ctx.h, ctypes.byref(p), ptr(a["idx"]), ptr(a["dist"]), ptr(a["dist2"]),
                                           ptr(a["qcounts"]), a["q_stride"], ptr(a["tcounts"]), a["t_stride"], ptr(a["back_idx"]),
                                           ptr(a["qangle"]), ptr(a["tangle"]), a["batch"], ptr(a["sel_q"]), ptr(a["sel_t"]),
                                           ptr(a["nsel"]), ptr(a["status"]), ptr(a["rot_hist"]))
    torch.cuda.synchronize()
    return rc


def assert_untouched(t):
    for k in OUT_KEYS:
        assert bool((t[k] == S8).all()), k


@pytest.mark.gpu
def test_gpu_select_rejects_bad_arguments(gpu_ctx):
    case = random_case(np.random.default_rng(11), [(100, 100), (50, 60)], 128, 128)
    t = select_tensors(case)
    for bad in (dict(max_dist=-1), dict(max_dist=257), dict(ratio=(0, 10)), dict(ratio=(11, 10)), dict(ratio=(8, 65536)),
                dict(ratio=(-1, -1)), dict(unique=2), dict(unique=-1), dict(rot_keep=31), dict(rot_keep=-1),
                dict(rot_min_pct=101), dict(rot_min_pct=-1)):
        assert raw_select(gpu_ctx, t, dict(ORBSLAM, **bad)) == -1, bad
    for bad in (dict(t_stride=65536), dict(q_stride=0), dict(q_stride=(1 << 22) + 1), dict(batch=-1), dict(batch=65536)):
        assert raw_select(gpu_ctx, t, ORBSLAM, **bad) == -1, bad
    for k in ("idx", "dist", "dist2", "qcounts", "tcounts", "back_idx", "qangle", "tangle") + OUT_KEYS:
        assert raw_select(gpu_ctx, t, ORBSLAM, **{k: t[k].cpu()}) == -1, ("host pointer", k)
    for k in ("idx", "dist", "qcounts", "tcounts", "sel_q", "sel_t", "nsel"):
        assert raw_select(gpu_ctx, t, ORBSLAM, **{k: None}) == -1, ("null pointer", k)
    assert_untouched(t)
    assert raw_select(gpu_ctx, t, ORBSLAM, batch=0) == 0                            # a no-op
    assert_untouched(t)
    assert raw_select(gpu_ctx, t, ORBSLAM) == 0                                     # and the call itself is accepted
    assert not bool((t["nsel"] == S8).all())


@pytest.mark.gpu
def test_gpu_angles_and_select_are_hipgraph_capturable(gpu_ctx):
    """Both calls have no workspace: captured into one graph (one stream, a linear chain) on a fresh context without a
    warm-up call of either, replayed twice with different inputs in the same tensors."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import orbAnglesBatch, selectMatchesBatch
    from test_orb_angles_batch import ref_angles
    from oracle import orc
    dev = torch.device("cuda:0")
    B, n, vstep, rows = 2, 96, 64, 48

    def inputs(seed):
        rng = np.random.default_rng(seed)
        img = rng.integers(0, 256, (2 * B, rows, vstep), dtype=np.uint8)          # B query pyramids, then B train pyramids
        kp = ((rng.integers(15, vstep - 15, (2 * B, n)) << 12) | rng.integers(15, rows - 15, (2 * B, n))).astype(np.uint32)
        cnt = arr([n, n - 7, n - 1, n])
        case = random_case(rng, [(n, n - 1), (n - 7, n)], n, n)
        case["dist"][:] = rng.integers(0, 60, (B, n))
        return img, kp, cnt, case

    img, kp, cnt, case = inputs(0)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        d = dict(img=T(img), kp=T(kp), cnt=T(cnt), idx=T(case["idx"]), dist=T(case["dist"]), dist2=T(case["dist2"]))
        ang = torch.zeros((2 * B, n), dtype=torch.uint8, device=dev)
        outs = dict(sel_q=torch.zeros((B, n), dtype=torch.int32, device=dev), sel_t=torch.zeros((B, n), dtype=torch.int32, device=dev),
                    nsel=torch.zeros((B,), dtype=torch.int32, device=dev), status=torch.zeros((B, n), dtype=torch.uint8, device=dev),
                    rot_hist=torch.zeros((B, 30), dtype=torch.int32, device=dev))
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            orbAnglesBatch(d["img"], d["kp"], d["cnt"], ang, ctx=ctx)
            selectMatchesBatch(d["idx"], d["dist"], d["dist2"], d["cnt"][:B], d["cnt"][B:], qangle=ang[:B], tangle=ang[B:], ctx=ctx,
                               **ORBSLAM, **outs)
        for seed in (0, 1):
            img, kp, cnt, case = inputs(seed)
            for k, v in (("img", img), ("kp", kp), ("cnt", cnt), ("idx", case["idx"]), ("dist", case["dist"]), ("dist2", case["dist2"])):
                d[k].copy_(T(v))
            ang.fill_(S8)
            for o in outs.values():
                o.zero_()
            g.replay()
            side.synchronize()
            a = ang.cpu().numpy()
            for b in range(2 * B):
                assert (a[b, :cnt[b]] == ref_angles(orc, img[b], kp[b, :cnt[b]])).all() and (a[b, cnt[b]:] == S8).all()
            c = dict(case, qc=cnt[:B], tc=cnt[B:], back=None, qa=a[:B], ta=a[B:])
            got = tuple(outs[k].cpu().numpy() for k in OUT_KEYS)
            sq, st, ns, status, hist = got
            for b in range(B):
                nq, nt = int(cnt[b]), int(cnt[B + b])
                eq, et, est, eh = ref_select(c["idx"][b, :nq], c["dist"][b, :nq], c["dist2"][b, :nq], nt, qa=a[b, :nq], ta=a[B + b, :nt],
                                             **ORBSLAM)
                assert int(ns[b]) == len(eq) and (sq[b, :len(eq)] == eq).all() and (st[b, :len(eq)] == et).all()
                assert (sq[b, len(eq):] == 0).all() and (status[b, :nq] == est).all() and (hist[b] == eh).all()
        ctx.close()
