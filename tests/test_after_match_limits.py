"""pislam_match_select_batch and pislam_orb_angles_batch at their block, chunk, batch and address limits (DESIGN.md
section 5.5); test_match_select.py and test_orb_angles_batch.py hold the semantics and the everyday shapes.

Selection: one workgroup of 1024 threads walks a pair's queries in blocks of 1024 and its train range in chunks of
16384.  The cases here have several blocks (the carry of the compaction), several blocks times several chunks (the
table is thrown out and filled again), the largest query index 2^22 - 1 in the claim key, the largest batch, and the
extremes of every input.  Angles: the circle mask pixel by pixel, more keypoints than one pass of the grid, more
pyramids than one launch, 12-bit coordinates in a batch that crosses 2^31 and 2^32 bytes, a pyramid stride with a gap.

Every expectation is bit-exact: `ref_select` for the selection (itself checked here against a plain loop), the oracle
for the angles.  Outputs are pre-filled with the sentinel and must be untouched past nq_b / nsel[b] / n_b."""
import functools

import numpy as np
import pytest

from test_match_select import (GRID, OFF, ORBSLAM, assert_untouched, check_select, random_case, raw_select,  # noqa: F401
                               ref_select, run_select, select_tensors, without)
from test_match_window import COUNT_INVALID, SENTINEL, clamp_count
from test_orb_angles_batch import check_angles, ref_angles, run_angles

S8 = SENTINEL & 0xFF
NONE = 0xFFFFFFFF
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
UNIQUE = dict(OFF, unique=1)
BLOCK, CHUNK = 1024, 16384                        # queries per compaction block, train indices per table chunk


def consistent_back(rng, case, b, share=0.5):
    """Row b of back_idx again after idx was edited: about `share` of the valid proposals are pointed back at."""
    qs = case["idx"].shape[1]
    nq, nt = clamp_count(case["qc"][b], qs), clamp_count(case["tc"][b], case["ts"])
    case["back"][b] = rng.integers(-1, qs, case["ts"])
    idx = case["idx"][b, :nq]
    ok = np.flatnonzero((idx >= 0) & (idx < nt))
    ok = ok[rng.random(len(ok)) < share]
    case["back"][b, idx[ok]] = ok


def clear_hot(case, b, hot, planted):
    """No query of pair b but the planted ones proposes a train index of `hot`."""
    stray = np.isin(case["idx"][b], hot)
    stray[planted] = False
    case["idx"][b, stray] = -1


# ---- 1. CPU: the vectorised reference against a plain loop -----------------------------------------------------------
def loop_select(idx, dist, dist2, nt, back, qa, ta, *, max_dist, ratio, unique, rot_keep, rot_min_pct):
    """The header's six steps, one query at a time: (selected queries, their train indices, status, histogram)."""
    nq = len(idx)
    status = [0] * nq
    best = {}                                                       # train index -> the smallest (dist, i) proposing it
    for i in range(nq):
        j, d = int(idx[i]), int(dist[i])
        if j < 0 or j >= nt:
            status[i] = 1
        elif d > max_dist:
            status[i] = 2
        elif ratio is not None and int(dist2[i]) != NONE and d * ratio[1] >= int(dist2[i]) * ratio[0]:
            status[i] = 3
        elif back is not None and int(back[j]) != i:
            status[i] = 4
        elif unique and (j not in best or (d, i) < best[j]):
            best[j] = (d, i)
    if unique:
        for i in range(nq):
            if status[i] == 0 and best[int(idx[i])] != (int(dist[i]), i):
                status[i] = 5
    hist = [0] * 30
    if rot_keep > 0:
        bins = {}
        for i in range(nq):
            if status[i] == 0:
                a, t = int(qa[i]), int(ta[int(idx[i])])
                if a >= 30 or t >= 30:
                    status[i] = 6
                else:
                    bins[i] = (a - t + 30) % 30
                    hist[bins[i]] += 1
        order = sorted(range(30), key=lambda k: (-hist[k], k))
        kept = {k for r, k in enumerate(order) if r < rot_keep and hist[k] >= 1 and 100 * hist[k] >= rot_min_pct * hist[order[0]]}
        for i, k in bins.items():
            if k not in kept:
                status[i] = 6
    sel = [i for i in range(nq) if status[i] == 0]
    return sel, [int(idx[i]) for i in sel], status, hist


def test_reference_equals_a_plain_loop_at_scale():
    """3000 queries on 200 train entries (15 proposals per train index): ref_select equals the per-query loop under
    every parameter set of GRID, and ORB-SLAM's settings with the cross-check meet every status code."""
    nq, nt = 3000, 200
    case = random_case(np.random.default_rng(3000), [(nq, nt)], nq, nt)
    case["dist"][0] = np.random.default_rng(1).integers(0, 70, nq)
    row = lambda k: None if case.get(k) is None else case[k][0]
    for name, params, drop in GRID:
        c = without(case, *drop)
        use_rot = params["rot_keep"] > 0
        kw = dict(params) if use_rot else dict(params, rot_keep=0)
        got = ref_select(c["idx"][0], c["dist"][0], c["dist2"][0], nt, back=c["back"] if c["back"] is None else c["back"][0],
                         qa=row("qa") if use_rot else None, ta=row("ta") if use_rot else None, **kw)
        sel, st, status, hist = loop_select(c["idx"][0], c["dist"][0], c["dist2"][0], nt,
                                            None if c["back"] is None else c["back"][0], row("qa"), row("ta"), **kw)
        assert got[0].tolist() == sel and got[1].tolist() == st, name
        assert got[2].tolist() == status and got[3].tolist() == hist, name
        if name == "orbslam+back":                   # (after a cross-check a train index has one proposal left: no 5)
            assert set(status) == {0, 1, 2, 3, 4, 6} and len(sel) > 20
        if name == "orbslam":
            assert set(status) == {0, 1, 2, 3, 5, 6} and len(sel) > 20
        if name == "unique":
            assert status.count(5) > 2000                                    # heavy contention


# ---- 2. more than one query block ----------------------------------------------------------------------------------
BLOCK_NQ = [1023, 1024, 1025, 2047, 2048, 2049, 4097, 5000, COUNT_INVALID]


@functools.lru_cache(maxsize=None)
def block_case():
    rng = np.random.default_rng(1024)
    case = random_case(rng, [(n, 1500) for n in BLOCK_NQ], 5000, 1500)
    case["idx"][7, 1024:2048] = -1                                           # block 1 of the 5000-query pair: nothing
    case["idx"][7, 2048:3072] = rng.integers(0, 1500, 1024)                  # block 2: everything, under OFF
    consistent_back(rng, case, 7)
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("name", [g[0] for g in GRID])
def test_gpu_select_query_blocks(gpu_ctx, name):
    """q_stride 5000: query counts on both sides of 1, 2 and 4 blocks of 1024, so the compaction carries its offset
    from block to block.  The last real pair has a block that selects nothing and, under OFF, one that selects all
    1024: carries of 0 and of 1024."""
    _, params, drop = next(g for g in GRID if g[0] == name)
    case = without(block_case(), *drop)
    got = run_select(gpu_ctx, case, **params)
    check_select(got, case, **params)
    sel_q, _, nsel, status, _ = got
    assert (status[7, 1024:2048] == 1).all() and int(nsel[8]) == 0
    before = int((status[7, :1024] == 0).sum())
    assert before > 0
    if name == "off":
        assert (status[7, 2048:3072] == 0).all()
        assert (sel_q[7, before:before + 1024] == np.arange(2048, 3072)).all()    # (block 1 added nothing)
        assert int(nsel[7]) > before + 1024
    assert int(nsel[6]) > 0 and status[6, 4096] != S8 and status[6, 4097] == S8


# ---- 3. several blocks times several chunks --------------------------------------------------------------------------
HOT = [0, 16383, 16384, 32767, 32768, 49151, 49152, 65534]
CONTENDERS = {0: (5, 1030, 2100, 4999), 1: (5, 1030, 2100, 4096), 2: (7, 1031, 1500, 2999), 4: (5, 1030, 2100, 4999)}


@functools.lru_cache(maxsize=None)
def chunk_case():
    """Pairs 0-2: random proposals over the whole train range (a); pair 3: block k proposes into chunk k % 4 only (b);
    pairs 0, 1, 2 and 4 carry the contests of (c): pair 4 with equal distances, the others with the last block winning.
    Returns (case, {pair: [(train, queries)]})."""
    rng = np.random.default_rng(65535)
    pairs = [(5000, 65535), (4097, 16385), (3000, 32768), (5000, 65535), (5000, 65535)]
    case = random_case(rng, pairs, 5000, 65535)
    case["dist"][:] = rng.integers(0, 60, case["dist"].shape)
    for k in range(5):                                                       # (b) 5 blocks on chunks 0, 1, 2, 3, 0
        c = k % 4
        lo, hi = c * CHUNK, min((c + 1) * CHUNK, 65535)
        q = slice(k * BLOCK, min((k + 1) * BLOCK, 5000))
        case["idx"][3, q] = rng.integers(lo, lo + 400, q.stop - q.start) if k % 2 else rng.integers(hi - 400, hi, q.stop - q.start)
    plants = {}
    for b, qq in CONTENDERS.items():
        nt = pairs[b][1]
        hot = [j for j in HOT if j < nt]
        plants[b] = []
        for n, j in enumerate(hot):                                           # contest n: the queries qq shifted by n
            q = np.array([qq[0] + n, qq[1] + n, qq[2] + n, qq[3] - n])
            case["idx"][b, q] = j
            case["dist"][b, q] = 6 if b == 4 else [9, 8, 7, 5]
            case["dist2"][b, q] = NONE
            plants[b].append((j, q))
        clear_hot(case, b, hot, np.concatenate([q for _, q in plants[b]]))
    for b in range(5):
        consistent_back(rng, case, b)
    return case, plants


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unique", "orbslam", "orbslam+back"])
def test_gpu_select_blocks_times_chunks(gpu_ctx, name):
    """t_stride 65535 with up to 5 query blocks and 4 table chunks: every block has proposals in every chunk, so each
    chunk is thrown out and filled again by the later blocks; in pair 3 consecutive blocks need different single chunks
    and skip the others; the planted contests have their contenders in different blocks."""
    _, params, drop = next(g for g in GRID if g[0] == name)
    case, plants = chunk_case()
    c = without(case, *drop)
    got = run_select(gpu_ctx, c, **params)
    check_select(got, c, **params)
    if name != "unique":
        return
    status = got[3]
    for b, contests in plants.items():
        assert len(contests) == (3 if b == 1 else 4 if b == 2 else 8)
        assert contests[0][1][3] == clamp_count(case["qc"][b], 5000) - 1     # the pair's last query is a contender
        for j, q in contests:
            assert q[0] < BLOCK <= q[1] and q[1] // BLOCK <= q[2] // BLOCK < q[3] // BLOCK      # the winner's block is its own
            want = [0, 5, 5, 5] if b == 4 else [5, 5, 5, 0]                  # equal distances: block 0; else the last block
            assert status[b, q].tolist() == want, (b, j, status[b, q])
    for k in range(5):                                                       # pair 3: the arrangement is what it claims
        live = case["idx"][3, k * BLOCK:(k + 1) * BLOCK]
        assert ((live // CHUNK) == k % 4).all()
        assert (status[3, k * BLOCK:min((k + 1) * BLOCK, 5000)] == 0).any()
    for b in (0, 2):                                                         # (a): every block selects from every chunk
        nq, nt = case["qc"][b], case["tc"][b]
        for k in range((int(nq) + BLOCK - 1) // BLOCK):
            blk = slice(k * BLOCK, min((k + 1) * BLOCK, int(nq)))
            chunks = set((case["idx"][b, blk][status[b, blk] == 0] // CHUNK).tolist())
            if blk.stop - blk.start > 100:
                assert chunks == set(range((int(nt) + CHUNK - 1) // CHUNK)), (b, k, chunks)


# ---- 4. the largest query index --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_case():
    """q_stride 2^22, one chunk of 16384 train entries, 256 proposals per train index; contests between a small query
    index and the largest ones.  Returns (case, {(pair, query): status under `unique`})."""
    Q = 1 << 22
    rng = np.random.default_rng(22)
    nqs = (Q, Q - 1023)
    case = dict(ts=CHUNK, idx=rng.integers(-1, CHUNK + 2048, (2, Q), dtype=np.int32), dist=rng.integers(0, 257, (2, Q), dtype=np.uint32),
                back=None, qa=rng.integers(0, 30, (2, Q), dtype=np.uint8), ta=rng.integers(0, 3, (2, CHUNK), dtype=np.uint8),
                qc=np.array(nqs, np.uint32), tc=np.array([CHUNK, CHUNK], np.uint32))
    case["dist2"] = np.where(rng.integers(0, 3, (2, Q)) == 0, NONE, case["dist"] + rng.integers(0, 120, (2, Q), dtype=np.uint32)).astype(np.uint32)
    hot = [100, 101, 102, 103, 104]
    want = {}
    for b, nq in enumerate(nqs):
        top = nq - 1
        contests = [(100, [(3, 256, 0), (top, 256, 5)]),                     # equal at the largest distance: the small index
                    (101, [(4, 256, 5), (top - 1, 255, 0)]),                 # the largest index but one wins by distance
                    (102, [(top - 2, 256, 0)]),                              # alone: its key is not the empty slot's value
                    (103, [(5, 7, 0), (top - 3, 7, 5), (top - 4, 7, 5)]),    # equal smaller distances
                    (104, [(top - 6, 0, 5), (top - 7, 0, 0), (6, 1, 5)])]    # distance 0: the key is the index alone
        planted = []
        for j, qq in contests:
            for i, d, st in qq:
                case["idx"][b, i], case["dist"][b, i], case["dist2"][b, i] = j, d, NONE
                want[b, i] = st
                planted.append(i)
        clear_hot(case, b, hot, np.array(planted))
    case["idx"][1, nqs[1]:] = 100                                            # beyond the count: would win every contest
    case["dist"][1, nqs[1]:] = 0
    return case, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unique", "orbslam256"])
def test_gpu_select_largest_query_index(gpu_ctx, name):
    """nq = 2^22 and 2^22 - 1023 with max_dist 256: the claim key dist << 23 | i at its largest, 256 << 23 | 2^22 - 1,
    stays apart from the empty slot and orders by distance first, index second."""
    params, drop = (UNIQUE, ("qa", "ta")) if name == "unique" else (dict(ORBSLAM, max_dist=256), ())
    case, want = wide_case()
    c = without(case, *drop)
    got = run_select(gpu_ctx, c, **params)
    check_select(got, c, **params)
    assert int(got[2][0]) > 1000 and int(got[2][1]) > 1000
    if name == "unique":
        for (b, i), st in want.items():
            assert got[3][b, i] == st, (b, i, got[3][b, i], st)
        assert got[3][0, (1 << 22) - 1] == 5 and got[3][0, (1 << 22) - 3] == 0


# ---- 5. the largest batch ------------------------------------------------------------------------------------------
def expected_rows(case, **params):
    """What a call leaves in sentinel-filled outputs, from ref_select pair by pair: (sel_q, sel_t, nsel, status, hist)."""
    B, qs = case["idx"].shape
    sel_q, sel_t = np.full((B, qs), SENTINEL, np.int32), np.full((B, qs), SENTINEL, np.int32)
    nsel, status, hist = np.zeros(B, np.int32), np.full((B, qs), S8, np.uint8), np.zeros((B, 30), np.int32)
    use_rot = params["rot_keep"] > 0
    for b in range(B):
        nq, nt = clamp_count(case["qc"][b], qs), clamp_count(case["tc"][b], case["ts"])
        eq, et, est, eh = ref_select(case["idx"][b, :nq], case["dist"][b, :nq], case["dist2"][b, :nq], nt,
                                     back=None if case["back"] is None else case["back"][b, :nt],
                                     qa=case["qa"][b, :nq] if use_rot else None, ta=case["ta"][b, :nt] if use_rot else None, **params)
        sel_q[b, :len(eq)], sel_t[b, :len(eq)], nsel[b], status[b, :nq], hist[b] = eq, et, len(eq), est, eh
    return sel_q, sel_t, nsel, status, hist


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["off", "orbslam"])
def test_gpu_select_largest_batch(gpu_ctx, name):
    """batch 65535 (65536 is refused: test_gpu_select_rejects_bad_arguments) of strides 8: pair b carries pattern b % 257
    of 257 small cases.  257 does not divide 65535, so a pair addressed at the wrong offset shows as a phase shift."""
    _, params, drop = next(g for g in GRID if g[0] == name)
    B, P, n = 65535, 257, 8
    rng = np.random.default_rng(257)
    counts = np.array([0, 1, 2, 3, 5, 7, 8, 8, 8, 9, 100, COUNT_INVALID], np.uint32)
    pairs = [(0, 5), (8, 0), (COUNT_INVALID, 8), (8, COUNT_INVALID), (9, 9), (8, 8)] + \
            [(int(rng.choice(counts)), int(rng.choice(counts))) for _ in range(P - 6)]
    pat = random_case(rng, pairs, n, n)
    pat["dist"][:] = rng.integers(0, 60, (P, n))
    pat = without(pat, *drop)
    exp = expected_rows(pat, **params)
    assert len({e.tobytes() for e in exp[3]}) > 90 and exp[2].max() >= 5 and (exp[2] == 0).sum() > 10   # patterns differ
    which = np.arange(B) % P
    case = {k: (v if v is None or k == "ts" else v[which]) for k, v in pat.items()}
    got = run_select(gpu_ctx, case, **params)
    for g, e, what in zip(got, exp, ("sel_q", "sel_t", "nsel", "status", "rot_hist")):
        bad = np.flatnonzero((g != e[which]).reshape(B, -1).any(axis=1))
        assert len(bad) == 0, (what, name, bad[:5], len(bad))


# ---- 6. input extremes -----------------------------------------------------------------------------------------------
BAD_DIST = (257, 511, 512, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def extremes_case():
    """One pair, one query per line.  Returns (case, rows): rows[label] = query index."""
    qs, ts, nt = 96, 80, 64
    idx, dist, dist2, qa = [], [], [], []
    ta, back = np.zeros(ts, np.uint8), np.full(ts, -1, np.int32)
    rows, trains = {}, iter(range(nt - 1))                                   # train nt - 1 is kept for the idx line

    def q(label, j, d, d2=NONE, a=None, point_back=True):
        i = len(idx)
        idx.append(j), dist.append(d), dist2.append(d2), qa.append(a)
        rows[label] = i
        if point_back and 0 <= j < nt:
            back[j] = i
        return i

    for d in BAD_DIST:                                   # a distance out of range first, so that a key of it that wrapped
        j = next(trains)                                 # would be the smaller one; then the honest query of the train
        q(("far", d), j, d, point_back=False)
        q(("honest", d), j, 256)
    q("d2 max", next(trains), 256, 0xFFFFFFFE)
    q("zero zero", next(trains), 0, 0)
    q("d2 none", next(trains), 256, NONE)
    q("1/65535 equal", next(trains), 1, 65535)           # 1 * 65535 >= 65535 * 1: fails under (1, 65535) alone
    q("1/65535 below", next(trains), 1, 65536)
    q("8/10 equal", next(trains), 8, 10)
    for j in (I32_MIN, -1, nt - 1, nt, ts - 1, ts, I32_MAX):                 # (nt <= j < t_stride is no match either)
        q(("idx", j), j, 3)
    for v in ("-1", "nq", "min", "i"):
        q(("back", v), next(trains), 5, point_back=False)
    q("qa 29", next(trains), 5, a=29)
    q("qa 30", next(trains), 5, a=30)
    q("qa ff", next(trains), 5, a=0xFF)
    for t in (29, 30, 0xFF):
        j = next(trains)
        ta[j] = t
        q(("ta", t), j, 5, a=2)
    plain = [i for i, a in enumerate(qa) if a is None and 0 <= idx[i] < nt and dist[i] <= 256]
    if len(plain) % 2:
        plain.append(q("filler", next(trains), 5))
    for n, i in enumerate(plain):                                            # two bins of equal count: 4 and 9
        qa[i] = 4 if n % 2 == 0 else 9
    qa = [0 if a is None else a for a in qa]
    nq = len(idx)
    assert nq < qs - 8
    for v, val in (("-1", -1), ("nq", nq), ("min", I32_MIN), ("i", rows["back", "i"])):
        back[idx[rows["back", v]]] = val
    pad = qs - nq                                                            # beyond the count: would win every contest
    case = dict(ts=ts, idx=np.array([idx + [0] * pad], np.int32), dist=np.array([dist + [0] * pad], np.uint32),
                dist2=np.array([dist2 + [NONE] * pad], np.uint32), qa=np.array([qa + [4] * pad], np.uint8), ta=ta[None],
                back=back[None], qc=np.array([nq], np.uint32), tc=np.array([nt], np.uint32))
    return case, rows


EXTREME_SETS = [("unique", UNIQUE, ("back", "qa", "ta")),
                ("ratio 1/1", dict(UNIQUE, ratio=(65535, 65535)), ("back", "qa", "ta")),
                ("ratio 1/65535", dict(UNIQUE, ratio=(1, 65535)), ("back", "qa", "ta")),
                ("ratio 8/10", dict(UNIQUE, ratio=(8, 10)), ("back", "qa", "ta")),
                ("back", UNIQUE, ("qa", "ta")),
                ("keep 1", dict(UNIQUE, rot_keep=1, rot_min_pct=0), ("back",)),
                ("keep 30, 0 %", dict(UNIQUE, rot_keep=30, rot_min_pct=0), ("back",)),
                ("keep 30, 100 %", dict(UNIQUE, rot_keep=30, rot_min_pct=100), ("back",)),
                ("orbslam", ORBSLAM, ("back",)),
                ("orbslam256+back", dict(ORBSLAM, max_dist=256), ()),
                ("max_dist 0", dict(UNIQUE, max_dist=0), ("back", "qa", "ta"))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [s[0] for s in EXTREME_SETS])
def test_gpu_select_input_extremes(gpu_ctx, name):
    """Distances beyond 9 bits against an honest query of the same train index (a wrapped key must never enter the
    table), the 64-bit ratio products at their largest, dist = dist2 = 0, idx and back_idx at the ends of int32, the
    angle codes 29 / 30 / 0xff on either side, and the histogram rules: two tied top bins, rot_keep 30, 0 and 100 %."""
    _, params, drop = next(s for s in EXTREME_SETS if s[0] == name)
    case, rows = extremes_case()
    c = without(case, *drop)
    got = run_select(gpu_ctx, c, **params)
    check_select(got, c, **params)
    status, hist = got[3][0], got[4][0]
    st = lambda label: int(status[rows[label]])
    if params["max_dist"] == 256:
        for d in BAD_DIST:
            assert st(("far", d)) == 2, (d, st(("far", d)))
            assert st(("honest", d)) in (0, 6), (d, st(("honest", d)))      # (6 only under a rotation check)
        assert [st(("idx", j)) for j in (I32_MIN, -1, 64, 79, 80, I32_MAX)] == [1] * 6 and st(("idx", 63)) in (0, 6)
    if name == "unique":
        assert all(st(("honest", d)) == 0 for d in BAD_DIST) and st(("idx", 63)) == 0
        assert st("zero zero") == 0 and st("d2 max") == 0
    if name.startswith("ratio"):
        assert st("zero zero") == 3 and st("d2 max") == 0 and st("d2 none") == 0 and st("1/65535 below") == 0
        assert st("1/65535 equal") == (3 if name == "ratio 1/65535" else 0)
        assert st("8/10 equal") == (0 if name == "ratio 1/1" else 3)           # 8 * 65535 >= 10 * 1 fails as well
    if name == "back":
        assert [st(("back", v)) for v in ("-1", "nq", "min", "i")] == [4, 4, 4, 0]
        assert all(st(("far", d)) == 2 and st(("honest", d)) == 0 for d in BAD_DIST)
    if name.startswith("keep"):
        assert hist[4] == hist[9] == hist.max() and hist[4] > 5 and hist[29] == 1 and hist[3] == 1 and hist.sum() == 2 * hist[4] + 2
        assert st("qa 30") == 6 and st("qa ff") == 6 and st(("ta", 30)) == 6 and st(("ta", 0xFF)) == 6
        sel_bins = set(((case["qa"][0][got[0][0, :got[2][0]]].astype(int) - case["ta"][0][got[1][0, :got[2][0]]]) % 30).tolist())
        assert sel_bins == {"keep 1": {4}, "keep 30, 0 %": {3, 4, 9, 29}, "keep 30, 100 %": {4, 9}}[name], sel_bins
        assert st("qa 29") == st(("ta", 29)) == (0 if name == "keep 30, 0 %" else 6)
    if name == "max_dist 0":
        assert st("zero zero") == 0 and int(got[2][0]) == 1


# ---- 7. the circle mask, pixel by pixel ----------------------------------------------------------------------------
def mosaic(value=255):
    """A 1023 x 1023 zero image of 31 x 31 tiles at pitch 32: tile n has its keypoint in the middle and one pixel of
    `value` at offset (n % 31 - 15, n // 31 - 15).  Returns (img, kp, dx, dy)."""
    n = np.arange(961)
    kx, ky = 15 + 32 * (n % 31), 15 + 32 * (n // 31)
    dx, dy = n % 31 - 15, n // 31 - 15
    img = np.zeros((1023, 1023), np.uint8)
    img[ky + dy, kx + dx] = value
    return img, ((kx << 12) | ky).astype(np.uint32), dx, dy


def test_oracle_sees_the_circle_mask_on_the_mosaic(orc):
    """The patch is the 793 offsets with dx^2 + dy^2 <= 250: a lit pixel among them gives its direction's bin, all 30
    occur; a lit pixel at one of the other 168 leaves the moments zero, which is bin 7."""
    img, kp, dx, dy = mosaic()
    inside = dx * dx + dy * dy <= 250
    assert int(inside.sum()) == 793
    bins = ref_angles(orc, img, kp)
    zero = int(ref_angles(orc, np.zeros((31, 31), np.uint8), [(15 << 12) | 15])[0])
    assert zero == 7
    assert set(bins[inside].tolist()) == set(range(30))
    assert (bins[~inside] == zero).all()
    at = lambda x, y: int(bins[(y + 15) * 31 + x + 15])
    for x, y in ((5, 15), (7, 14), (15, 5), (14, 7)):                        # the rim, away from bin 7's own direction
        assert at(x, y) != zero and at(-x, -y) != zero and at(x, y) != at(-x, -y)
        out = (x + 1, y) if y > x else (x, y + 1)
        assert at(*out) == zero and at(-out[0], -out[1]) == zero
    img1, _, _, _ = mosaic(1)
    assert (ref_angles(orc, img1, kp) == bins).all()                         # the bin is the direction's, whatever the value


@pytest.mark.gpu
def test_gpu_angles_single_pixel_mosaic(gpu_ctx, orc):
    """The mosaic with pixel value 255, with value 1 and inverted (negative moments of large magnitude) as a batch of
    three, each image with its own expectation."""
    img, kp, dx, dy = mosaic()
    imgs = np.stack([img, mosaic(1)[0], 255 - img])
    kps = np.stack([kp, kp, kp])
    got = run_angles(gpu_ctx, imgs, kps, [961] * 3)
    check_angles(orc, got, imgs, kps, [961] * 3)
    inside = dx * dx + dy * dy <= 250
    assert set(got[0, inside].tolist()) == set(range(30)) and (got[0, ~inside] == 7).all()
    assert (got[2] != got[0]).any()


# ---- 8. more keypoints than one pass of the grid ---------------------------------------------------------------------
def random_positions(rng, shape, limit):
    """Keypoint words with random score bits: positions 0 .. limit - 1 in x and y."""
    return ((rng.integers(0, 256, shape) << 24) | (rng.integers(0, limit, shape) << 12) | rng.integers(0, limit, shape)).astype(np.uint32)


@pytest.mark.gpu
def test_gpu_angles_more_keypoints_than_one_grid_pass(gpu_ctx, orc):
    """The grid of a call has min(ceil(stride / 4), 65535) workgroups of 4 waves for batch 1 and, per pyramid,
    min(ceil(stride / 4), ceil(16 * CUs / batch)) for a larger batch; a workgroup strides over further keypoints.
    (a) batch 1, stride = count = 4 * 65535 + 41: the last 41 keypoints are a second pass.  (b) batch 7, stride 8192:
    586 workgroups per pyramid on 256 CUs, so 2344 keypoints per pass and four passes for a full list; ragged counts."""
    rng = np.random.default_rng(8)
    stride = 262144 + 37
    assert stride > 4 * 65535
    img = rng.integers(0, 256, (1, 256, 256), dtype=np.uint8)
    kp = random_positions(rng, (1, stride), 272)                             # about one in ten leaves the image
    got = run_angles(gpu_ctx, img, kp, [stride])
    check_angles(orc, got, img, kp, [stride])
    assert (got[0, 4 * 65535:] < 30).any() and (got[0] == 0xFF).any() and set(got[0][got[0] < 30].tolist()) == set(range(30))
    counts = [0, 1, 4, 8191, 8192, 9000, COUNT_INVALID]
    img = rng.integers(0, 256, (7, 256, 256), dtype=np.uint8)
    kp = random_positions(rng, (7, 8192), 272)
    got = run_angles(gpu_ctx, img, kp, counts)
    check_angles(orc, got, img, kp, counts)
    assert (got[0] == S8).all() and (got[6] == S8).all() and got[3, 8190] != S8 and got[3, 8191] == S8


# ---- 9. more pyramids than one launch --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_angles_more_pyramids_than_one_launch(gpu_ctx, orc):
    """batch 65537 of 31 x 31 pyramids (the smallest allowed), stride 2: a launch covers 65535 pyramids, so the last two
    are a second launch whose four pointers are offset by hand.  Pyramid b is image b % 61 of 61 (the second launch
    starts at phase 21); counts cycle through 1, 2, 5, 0 and PISLAM_COUNT_INVALID."""
    B, P = 65537, 61
    rng = np.random.default_rng(61)
    pat = rng.integers(0, 256, (P, 31, 31), dtype=np.uint8)
    centre = (15 << 12) | 15
    bins = np.array([ref_angles(orc, pat[p], [centre])[0] for p in range(P)], np.uint8)
    assert len(set(bins.tolist())) >= 15 and len({bins[0], bins[21], bins[22]}) == 3 and (bins < 30).all()
    which = np.arange(B) % P
    counts = np.array([1, 2, 5, 0, COUNT_INVALID], np.uint32)[np.arange(B) % 5]
    n = np.where(counts == COUNT_INVALID, 0, np.minimum(counts, 2))
    kp = np.empty((B, 2), np.uint32)
    kp[:, 0], kp[:, 1] = (0x11 << 24) | centre, (0xEE << 24) | centre
    exp = np.where(np.arange(2)[None, :] < n[:, None], bins[which][:, None], S8).astype(np.uint8)
    got = run_angles(gpu_ctx, pat[which], kp, counts)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert len(bad) == 0, (bad[:5], len(bad), got[bad[:5]], exp[bad[:5]])
    assert got[65534].tolist() == [S8, S8]                                   # count invalid: not written
    assert got[65535].tolist() == [bins[21], S8] and got[65536].tolist() == [bins[22], bins[22]]


# ---- 10. 12-bit coordinates across 2^31 and 2^32 bytes -------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_angles_12_bit_coordinates_past_4_gib(gpu_ctx, orc):
    """256 pyramids of 4111 x 4111 bytes (4.33 GB, the narrowest buffer in which x = 4095 is a valid position): pyramid
    127 straddles 2^31 bytes and pyramid 254 straddles 2^32.  Pyramids 0, 127, 128, 254 and 255 are random and have
    keypoints at the four corners of the valid range; every other pyramid is zero with count 0."""
    import torch
    side, B, stride = 4111, 256, 64
    size = side * side
    assert 127 * size < 1 << 31 < 128 * size and 254 * size < 1 << 32 < 255 * size
    live = (0, 127, 128, 254, 255)
    rng = np.random.default_rng(4095)
    corners = [(15, 15), (4095, 15), (15, 4095), (4095, 4095), (4095, 2000), (2000, 4095), (4094, 4094)]
    kp = np.zeros((B, stride), np.uint32)
    for b in live:
        x, y = rng.integers(15, 4096, stride), rng.integers(15, 4096, stride)
        x[:len(corners)], y[:len(corners)] = np.array(corners).T
        kp[b] = (rng.integers(0, 256, stride) << 24) | (x << 12) | y
    counts = np.zeros(B, np.uint32)
    counts[list(live)] = stride
    dev = torch.device("cuda:0")
    d_pyr = ang = None
    try:
        d_pyr = torch.zeros((B, side, side), dtype=torch.uint8, device=dev)
        gen = torch.Generator(device=dev).manual_seed(4111)
        imgs = {}
        for b in live:
            d_pyr[b] = torch.randint(0, 256, (side, side), dtype=torch.uint8, device=dev, generator=gen)
            imgs[b] = d_pyr[b].cpu().numpy()
        from pislam_amd.frontend import orbAnglesBatch
        ang = torch.full((B, stride), S8, dtype=torch.uint8, device=dev)
        orbAnglesBatch(d_pyr, torch.from_numpy(kp.view(np.int32)).to(dev), torch.from_numpy(counts.view(np.int32)).to(dev), ang, ctx=gpu_ctx)
        torch.cuda.synchronize()
        got = ang.cpu().numpy()
    finally:
        d_pyr = ang = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    for b in range(B):
        if b in live:
            exp = ref_angles(orc, imgs[b], kp[b])
            assert (exp < 30).all() and len(set(exp.tolist())) > 10
            assert (got[b] == exp).all(), (b, np.flatnonzero(got[b] != exp)[:5])
        else:
            assert (got[b] == S8).all(), ("a pyramid of count 0 was written", b)
    assert any((imgs[a] != imgs[b]).any() for a in live for b in live if a < b)


@pytest.mark.gpu
def test_gpu_angles_last_valid_position_of_a_4096_buffer(gpu_ctx, orc):
    """vstep = rows = 4096: x or y of 4080 is the last valid position, 4081 gives 0xff and reads nothing."""
    rng = np.random.default_rng(4096)
    img = rng.integers(0, 256, (1, 4096, 4096), dtype=np.uint8)
    inside = [(4080, 4080), (4080, 15), (15, 4080), (4080, 2000), (2000, 4080)]
    outside = [(4081, 2000), (2000, 4081), (4081, 4081), (4081, 4080), (4080, 4081), (4095, 4095), (4095, 15), (15, 4095)]
    pts = inside + outside
    kp = np.array([[(0x5C << 24) | (x << 12) | y for x, y in pts]], np.uint32)
    got = run_angles(gpu_ctx, img, kp, [len(pts)])
    check_angles(orc, got, img, kp, [len(pts)])
    assert (got[0, :len(inside)] < 30).all() and (got[0, len(inside):] == 0xFF).all()


# ---- 11. a pyramid stride larger than the image --------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_angles_pyramid_stride_with_a_gap(gpu_ctx, orc):
    """The C entry with pyramid_stride = rows * vstep + 4097: three dark pyramids cut from one flat buffer whose gaps
    hold 0xff, keypoints on the first and last valid rows next to the gaps."""
    import torch
    from pislam_amd.capi import ptr
    rows, vstep, B, n = 48, 64, 3, 40
    pstride = rows * vstep + 4097
    rng = np.random.default_rng(4097)
    flat = np.full(B * pstride, 0xFF, np.uint8)
    imgs = rng.integers(0, 64, (B, rows, vstep), dtype=np.uint8)
    for b in range(B):
        flat[b * pstride:b * pstride + rows * vstep] = imgs[b].ravel()
    x, y = rng.integers(15, vstep - 15, (B, n)), rng.integers(15, rows - 15, (B, n))
    y[:, 0:8], y[:, 8:16] = 15, rows - 16
    x[:, 0], x[:, 8], x[:, 1], x[:, 9] = 15, 15, vstep - 16, vstep - 16
    kp = ((x << 12) | y).astype(np.uint32)
    counts = np.array([n, n - 3, n], np.uint32)
    dev = torch.device("cuda:0")
    d = [torch.from_numpy(a).to(dev) for a in (flat, kp.view(np.int32), counts.view(np.int32))]
    ang = torch.full((B, n), S8, dtype=torch.uint8, device=dev)
    rc = gpu_ctx.lib.pislam_orb_angles_batch(gpu_ctx.h, ptr(d[0]), vstep, rows, pstride, ptr(d[1]), ptr(d[2]), n, B, ptr(ang))
    torch.cuda.synchronize()
    assert rc == 0
    got = ang.cpu().numpy()
    check_angles(orc, got, imgs, kp, counts)
    packed = run_angles(gpu_ctx, imgs, kp, counts)                           # the same pyramids back to back
    assert (packed == got).all()
    wrong = np.stack([flat[b * rows * vstep:(b + 1) * rows * vstep].reshape(rows, vstep) for b in range(B)])
    assert any((ref_angles(orc, wrong[b], kp[b]) != got[b]).any() for b in (1, 2))   # the packed stride would show
