"""Key-frame database at its hard limits (pislam_bowdb_kernels.h): accumulate slices of 24576 ids and their packed
16-bit `common` plane, selection slices of 8192 ids, the 2048-entry queue of long posting lists, the merge that is full at
128 x 64 keys, the scan that is full at 2^24 words, counts on add and query, the weight call at stride 16384 and outside
its contract, the out-of-contract guarantee of the query, and two databases that share one context (one of them
captured into a hipGraph at the largest LDS size).

Every case is BUILT by a plain function (NumPy only, no torch, no device) that also computes what the library must
return, with `ref_query_fast`: a dense NumPy statement of the query that shares no code with the library and is proven
against test_bow_database.ref_query (the explicit join) on the CPU.  test_limit_cases_exercise_what_they_claim asserts,
from the reference alone, that each case reaches the branch it is meant for; the GPU tests replay the cases and compare
bit for bit.  The launch plan is restated here from include/pislam_hip.h and DESIGN.md section 5.5, not imported."""
import functools

import numpy as np
import pytest

from test_bow import COUNT_INVALID, T, dev, filled, host
from test_bow_database import Q24, RefDb, frame, ref_query, ref_weights
from test_match_window import SENTINEL, clamp_count

ACC_MAX_SLICE = 24576        # ids per accumulate workgroup (6 bytes of LDS each)
SEL_SLICE = 8192             # ids per selection workgroup
LONG = 1024                  # a posting list longer than this is walked by the whole workgroup ...
QUEUE = 2048                 # ... if it is among the first 2048 such lists of its query
SCAN_CHUNK = 16384           # words per scan workgroup


def plan(capacity):
    """(accumulate slices, ids per slice, selection slices) of a query against `capacity` key frames."""
    slices = -(-capacity // ACC_MAX_SLICE)
    return slices, (-(-capacity // slices) + 1) & ~1, -(-capacity // SEL_SLICE)


# ---- the second reference: dense NumPy ---------------------------------------------------------------------------------
class DenseDb:
    """Key frames as two int64 planes [capacity][stride] (word -1 past a frame's entries); ids in order of addition."""

    def __init__(self, nwords, stride, capacity):
        self.nwords, self.stride, self.capacity, self.size = nwords, stride, capacity, 0
        self.word = np.full((capacity, stride), -1, np.int64)
        self.val = np.zeros((capacity, stride), np.int64)
        self.alive = np.zeros(capacity, bool)

    def add(self, word, val):
        """Rows [b][s] (word -1 past the entries); a row longer than the database's stride keeps its first entries."""
        b, k = word.shape[0], min(word.shape[1], self.stride)
        if self.size + b > self.capacity:
            raise ValueError("capacity")
        first = self.size
        self.word[first:first + b, :k], self.val[first:first + b, :k] = word[:, :k], np.where(word[:, :k] >= 0, val[:, :k], 0)
        self.alive[first:first + b] = True
        self.size += b
        return first

    def remove(self, ids):
        ids = np.asarray(ids, np.int64)
        if len(set(ids.tolist())) != len(ids) or (ids < 0).any() or (ids >= self.size).any() or not self.alive[ids].all():
            raise ValueError("id")
        self.alive[ids] = False


def dense_of(db):
    if isinstance(db, DenseDb):
        return db
    d = DenseDb(db.nwords, db.stride, max(1, len(db.frames)))
    for k, (w, v) in enumerate(db.frames):
        d.word[k, :len(w)], d.val[k, :len(w)] = w, v
    d.size = len(db.frames)
    d.alive[:d.size] = db.alive
    return d


_TABLE = {}                                                          # one scratch table of -1 per size (left all -1)


def ref_query_fast(db, qw, qv, limit=None, pct=80, topk=16, want_all=True):
    """ref_query's tuple, computed for all key frames at once: the query is scattered into a table over the words
    (weight, or -1 for a word it does not hold), every stored entry looks its word up, `common` and `score` are row sums
    in int64, the selection is one lexsort on (-score, id).  `db` is a RefDb or a DenseDb.  want_all=False leaves the
    sixth element (the dict of all eligible key frames) None."""
    d = dense_of(db)
    n = d.size
    W, V = d.word[:n], d.val[:n]
    qw, qv = np.asarray(qw, np.int64), np.asarray(qv, np.int64)
    hi = min(d.nwords, int(W.max(initial=-1)) + 1)                   # no indexed entry holds a word at or above hi
    common, score = np.zeros(n, np.int64), np.zeros(n, np.int64)
    if hi > 0 and len(qw):
        tab = _TABLE.get(hi)
        if tab is None:
            _TABLE.clear()
            tab = _TABLE[hi] = np.full(hi, -1, np.int64)
        keep = qw < hi
        tab[qw[keep]] = qv[keep]
        inside = (W >= 0) & (W < hi)
        qe = tab[np.where(inside, W, 0)]
        hit = inside & (qe >= 0)
        common, score = hit.sum(1), np.where(hit, np.minimum(V, qe), 0).sum(1)
        tab[qw[keep]] = -1
    ids = np.arange(n)
    elig = d.alive[:n] & (ids < (n if limit is None else limit))
    max_common = int(common[elig].max(initial=0))
    cand = np.flatnonzero(elig & (common >= 1) & (common * 100 >= pct * max_common))
    order = cand[np.lexsort((cand, -score[cand]))][:topk]
    pad = topk - len(order)
    cs = {int(k): (int(common[k]), int(score[k])) for k in np.flatnonzero(elig)} if want_all else None
    return ([*order.tolist(), *[-1] * pad], [*score[order].tolist(), *[0] * pad], [*common[order].tolist(), *[0] * pad],
            max_common, len(cand), cs)


def test_fast_reference_against_the_join():
    """ref_query_fast against ref_query on 300 small random databases: dead ids, every id_limit form, pct 0 / 80 / 100,
    ties (few distinct weights), words at and above nwords, frames and queries longer than their stride, empty queries
    and empty databases."""
    rng = np.random.default_rng(31)
    seen = dict(dead=0, ties=0, over=0, clamped=0, empty_q=0, fewer=0, more=0, filtered=0, nolimit=0, nonpos=0, beyond=0)
    for trial in range(300):
        nwords, stride = int(rng.integers(1, 40)), int(rng.integers(1, 9))
        nkf = int(rng.integers(0, 30))
        ref = RefDb(nwords, stride, max(1, nkf))
        frames = []
        for _ in range(nkf):
            n = int(rng.integers(0, min(stride + 3, nwords + 5) + 1))
            w = rng.choice(nwords + 5, n, replace=False)
            frames.append(frame(w, rng.choice([0, 5, 5, 9, 1000], n)))
            seen["clamped"] += n > stride
            seen["over"] += bool((w[:stride] >= nwords).any())
        ref.add(frames)
        if nkf:
            dead = rng.choice(nkf, int(rng.integers(0, nkf // 3 + 1)), replace=False)
            ref.remove(dead)
            seen["dead"] += len(dead) > 0
        qstride = int(rng.integers(1, 12))
        for q in range(4):
            n = 0 if q == 3 and trial % 3 == 0 else int(rng.integers(0, min(qstride + 3, nwords + 5) + 1))
            w = rng.choice(nwords + 5, n, replace=False)[:qstride]          # the query's own stride clamps it
            v = rng.choice([0, 5, 7, 9, 2000], len(w))
            limit = [None, int(rng.integers(1, nkf + 3)), 0, -5, nkf][int(rng.integers(0, 5))]
            pct, topk = [0, 80, 100][int(rng.integers(0, 3))], [1, 2, 5, 16][int(rng.integers(0, 4))]
            a, b = ref_query(ref, w, v, limit, pct, topk), ref_query_fast(ref, w, v, limit, pct, topk)
            assert a == b, (trial, q, a[:5], b[:5])
            live = [s for i, s in zip(a[0], a[1]) if i >= 0]
            seen["ties"] += len(set(live)) < len(live)
            seen["empty_q"] += len(w) == 0
            seen["fewer"] += 0 < a[4] < topk
            seen["more"] += a[4] > topk
            seen["filtered"] += any(c >= 1 and c * 100 < pct * a[3] for c, _ in a[5].values())
            seen["nolimit"] += limit is None
            seen["nonpos"] += limit is not None and limit <= 0
            seen["beyond"] += limit is not None and limit > nkf
    assert all(v >= 10 for v in seen.values()), seen


# ---- cases: plain data and the expected results -----------------------------------------------------------------------
def gpu_rows(word, val, counts=None):
    """uint32 [B][S] word / weight arrays (SENTINEL past the entries) and counts of dense int64 rows."""
    used = word >= 0
    n = used.sum(1) if counts is None else np.asarray(counts)
    return (np.where(used, word, SENTINEL).astype(np.uint32), np.where(used, val, SENTINEL).astype(np.uint32),
            n.astype(np.uint32))


def rows(entries, stride):
    """Dense rows of a list of (words, weights)."""
    word, val = np.full((len(entries), stride), -1, np.int64), np.zeros((len(entries), stride), np.int64)
    for b, (w, v) in enumerate(entries):
        word[b, :len(w)], val[b, :len(w)] = w, v
    return word, val


class Case:
    """A database shape and a list of steps ("add", gpu arrays, first id) / ("remove", ids) / ("query", gpu arrays, topk,
    pct, limits, expected rows, candidates per query, label), recorded while the reference runs them."""

    def __init__(self, nwords, stride, capacity):
        self.ref, self.steps, self.notes = DenseDb(nwords, stride, capacity), [], {}

    def add(self, word, val, gpu=None):
        """`gpu`: the arrays the device gets when they differ from the dense rows (counts below the entries)."""
        self.steps.append(("add", gpu or gpu_rows(word, val), self.ref.add(word, val)))

    def remove(self, ids):
        self.ref.remove(ids)
        self.steps.append(("remove", [int(i) for i in ids]))

    def query(self, word, val, topk, pct, limits=None, what="", gpu=None):
        exp, ncand = [], []
        for b in range(len(word)):
            used = word[b] >= 0
            r = ref_query_fast(self.ref, word[b][used], val[b][used], None if limits is None else int(limits[b]), pct, topk,
                               want_all=False)
            exp.append([r[0], r[1], r[2], r[3]])
            ncand.append(r[4])
        self.steps.append(("query", gpu or gpu_rows(word, val), topk, pct, None if limits is None else np.asarray(limits, np.int32),
                           exp, ncand, what))
        return exp, ncand


def gpu_query_arrays(db, arrays, topk, pct, limits):
    import torch
    word, val, n = arrays
    B = len(n)
    outs = [filled((B, topk)), filled((B, topk)), filled((B, topk)), filled((B,))]
    db.query(T(word), T(val), T(n), topk=topk, min_common_pct=pct, id_limit=None if limits is None else T(limits),
             top_id=outs[0], top_score=outs[1], top_common=outs[2], max_common=outs[3])
    torch.cuda.synchronize()
    return [host(o) for o in outs]


def compare(got, exp, what):
    for b, e in enumerate(exp):
        g = [got[0][b].view(np.int32).tolist(), got[1][b].tolist(), got[2][b].tolist(), int(got[3][b])]
        assert g == e, (what, b, g, e)


def run_case(ctx, case):
    from pislam_amd.frontend import BowDatabase
    ref = case.ref
    db = BowDatabase(ref.nwords, ref.stride, ref.capacity, ctx=ctx)
    try:
        for step in case.steps:
            if step[0] == "add":
                assert db.add(*[T(a) for a in step[1]]) == step[2]
            elif step[0] == "remove":
                db.remove(step[1])
            else:
                _, arrays, topk, pct, limits, exp, _, what = step
                compare(gpu_query_arrays(db, arrays, topk, pct, limits), exp, what)
        assert db.size == ref.size
    finally:
        db.close()


# growth across the slice boundaries
GROW_STRIDE, GROW_WORDS, GROW_TOPK = 4, 256, 32


@functools.lru_cache(maxsize=None)
def growth_frames(capacity):
    """`capacity` key frames of four words.  Background frames hold words 16 .. 255 with weights from a small set.  At
    every boundary b (the multiples of 8192 and the accumulate slice start) id b holds word 0 and three background
    words ("one": common 1 with the query 0 1 2 3) and ids b - 1 and b + 1 hold exactly the words 0 1 2 3 ("full":
    common 4), as does the last id of every size the database is grown through.  b is even, so b and b + 1 share a dword
    of the packed common plane."""
    rng = np.random.default_rng([21, capacity])
    _, sl, _ = plan(capacity)
    sizes = [8191, 8192, 8193, sl - 1, sl, sl + 1, capacity - 1, capacity]
    bounds = sorted({sl} | set(range(SEL_SLICE, capacity, SEL_SLICE)))
    base, step = rng.integers(0, 240, capacity), rng.choice([1, 7, 11, 13, 17, 19, 23], capacity)   # (coprime to 240)
    word = 16 + (base[:, None] + step[:, None] * np.arange(GROW_STRIDE)) % 240
    val = rng.choice([1000, 2000, 3000, 5000], (capacity, GROW_STRIDE))
    one = [b for b in bounds if b < capacity]
    full = {}
    for i in [s - 1 for s in sizes] + [b - 1 for b in bounds]:
        full[i] = Q24 // 4
    for b in bounds:
        full[b + 1] = Q24 // 8
    for i, v in full.items():
        if 0 <= i < capacity and i not in one:
            word[i], val[i] = np.roll([0, 1, 2, 3], i), v
    word[one, 0], val[one, 0] = 0, Q24 // 4
    return word, val, sizes, bounds, one, sorted(i for i in full if 0 <= i < capacity and i not in one)


@functools.lru_cache(maxsize=None)
def growth_case(capacity):
    word, val, sizes, bounds, one, full = growth_frames(capacity)
    rng = np.random.default_rng([22, capacity])
    _, sl, _ = plan(capacity)
    case = Case(GROW_WORDS, GROW_STRIDE, capacity)
    case.notes.update(sizes=sizes, bounds=bounds, slice=sl, all_rows=[])
    q_all = ([3, 0, 2, 1], [Q24 // 4] * 4)                            # one: common 1, full: common 4
    for k, size in enumerate(sizes):
        case.add(word[case.ref.size:size], val[case.ref.size:size])
        forms = [size, sl, sl - 1, sl + 1, SEL_SLICE, 0, -5]
        entries, limits = [], []
        for j, lim in enumerate(forms):
            near = [b for b in bounds if b < size] or [size]
            src = int(near[j % len(near)]) - 1 - j                    # a background frame next to a boundary, as stored
            entries += [q_all, (word[src], np.full(GROW_STRIDE, 2500))]
            limits += [lim, lim]
        entries += [([0, 2], [Q24 // 4, Q24 // 16]), ([300, 0, 5000, 1], [7, Q24 // 2, 7, 9]), ([], []),
                    (rng.integers(16, 256, 1), [4000])]
        limits += [size, size, size, size]
        qw, qv = rows(entries, GROW_STRIDE)
        exp, _ = case.query(qw, qv, GROW_TOPK, 0, None, ("grow", capacity, size, "pct 0"))
        case.notes["all_rows"].append((size, exp[0]))
        case.query(qw, qv, GROW_TOPK, 80, limits, ("grow", capacity, size, "pct 80, limits"))
        case.query(qw, qv, 5, 0, limits, ("grow", capacity, size, "pct 0, limits, topk 5"))
        if k == 3:
            case.remove([SEL_SLICE])                                  # a boundary id dies between two steps
        if k == 5:
            case.remove([sl - 1, 100])
    return case


# long posting lists and the queue
LONG_WORDS, LONG_CAP = 2200, 1100


@functools.lru_cache(maxsize=None)
def long_case():
    """Key frame k holds word w exactly when k < lens[w]: lens[w] is the length of w's posting list."""
    rng = np.random.default_rng(23)
    lens = np.concatenate([rng.choice([1025, 1100], 2100), [1] * 30, [1023] * 35, [1024] * 35])
    lens = lens[rng.permutation(LONG_WORDS)]
    present = np.arange(LONG_CAP)[:, None] < lens[None, :]
    keys = rng.random((LONG_CAP, LONG_WORDS))
    keys[~present] = 2.0
    order = np.argsort(keys, axis=1)                                  # each frame's words in random order, absent ones last
    used = np.arange(LONG_WORDS)[None, :] < present.sum(1)[:, None]
    word = np.where(used, order, -1)
    val = np.where(used, rng.choice([1000, 2000, 4000, 7000], word.shape), 0)     # 2200 * 7000 < 2^24
    case = Case(LONG_WORDS, LONG_WORDS, LONG_CAP)
    case.add(word[:600], val[:600])
    case.add(word[600:], val[600:])
    long_ids, short_ids = np.flatnonzero(lens > LONG), np.flatnonzero(lens <= LONG)

    def q(nlong, nshort):
        w = np.concatenate([rng.choice(long_ids, nlong, replace=False), rng.choice(short_ids, nshort, replace=False)])
        rng.shuffle(w)
        return w, rng.choice([500, 3000, 7000], len(w))

    edge = np.concatenate([np.flatnonzero(lens == 1024), np.flatnonzero(lens == 1025)[:40]])
    rng.shuffle(edge)
    entries = [q(2100, 100), q(2048, 60), (edge, rng.choice([500, 3000, 7000], len(edge))), q(2049, 60), q(2049, 0)]
    case.notes.update(lens=lens, queries=[e[0] for e in entries])
    qw, qv = rows(entries, LONG_WORDS)
    for topk in (1, 16, 64):
        for pct in (0, 80):
            case.query(qw, qv, topk, pct, None, ("long", topk, pct))
    return case


# the full merge
MERGE_SIZE = 127 * SEL_SLICE + 1000
MERGE_PLANTED = [0, 20, 40, 60, 70, 90, 100, 127]                  # selection slices that hold the largest weights


@functools.lru_cache(maxsize=None)
def merge_case():
    """2^20 capacity, stride 1: 128 selection slices of 64 partial keys each, all eight register rows of the merge.
    Background frames hold one of the words 8 .. 63 (or 70, which is not indexed) with a weight of 100 .. 400; the words
    0 .. 7 are rare: the planted frames (word 5, weights 5000 .. 6000, six in each slice of MERGE_PLANTED) and thirty
    sparse frames of weight 400 in each of the slices 0, 60 and 127.  Slices 1 .. 15 hold no rare word, so a query for
    rare words leaves their partial lists empty."""
    rng = np.random.default_rng(24)
    N = MERGE_SIZE
    word = rng.integers(8, 64, (N, 1))
    word[rng.random(N) < 0.01] = 70
    val = rng.choice([100, 200, 300, 400], (N, 1))
    planted = []
    for s in MERGE_PLANTED:
        ids = s * SEL_SLICE + rng.choice(1000, 6, replace=False)
        word[ids, 0], val[ids, 0] = 5, rng.choice([5000, 5500, 6000], 6)
        planted += ids.tolist()
    for s in (0, 60, 127):
        ids = s * SEL_SLICE + 1000 - 1 - rng.choice(500, 30, replace=False)       # (apart from the planted: the last id too)
        word[ids, 0], val[ids, 0] = rng.choice([5, 1, 2], 30), 400
    word[N - 1, 0], val[N - 1, 0] = 5, 400
    case = Case(64, 1, 1 << 20)
    case.add(word[:600000], val[:600000])
    case.add(word[600000:], val[600000:])
    rare, mixed, flat = ([5, 1, 2, 3], [10000] * 4), ([10, 5, 70, 11], [250, 10000, 9, 350]), ([20, 21, 22, 23], [150] * 4)
    qw, qv = rows([rare, mixed, flat, rare, mixed, rare], 4)
    inside = 127 * SEL_SLICE + 500
    limits = [1 << 20, 127 * SEL_SLICE, inside, 127 * SEL_SLICE, 1 << 20, inside]
    case.notes["first"] = case.query(qw, qv, 64, 0, None, "merge, topk 64, pct 0")
    case.query(qw, qv, 64, 80, limits, "merge, topk 64, pct 80, limits")
    case.query(qw, qv, 1, 0, limits, "merge, topk 1, pct 0, limits")
    case.query(qw, qv, 1, 80, None, "merge, topk 1, pct 80")
    dead = sorted(set(rng.choice(N, 990, replace=False).tolist()) | set(planted[:3] + planted[-3:] + planted[20:24]))
    case.remove(dead)
    case.notes["after"] = case.query(qw, qv, 64, 0, limits, "merge, removed, limits")
    case.query(qw, qv, 64, 80, None, "merge, removed, pct 80")
    case.notes.update(planted=planted, dead=dead)
    return case


# scan chunk edges
SCAN_STRIDE, SCAN_CAP = 8, 64


@functools.lru_cache(maxsize=None)
def scan_case(nwords):
    rng = np.random.default_rng([25, nwords])
    special = sorted({0, 16383, 16384, nwords - 1})                  # (16384 is not a word of the 16384-word database)
    pool = np.unique(np.concatenate([special, rng.integers(0, nwords, 20), [nwords, nwords + 3, (1 << 24) + 5]]))

    def draw(count):
        out = []
        for _ in range(count):
            w = np.unique(np.concatenate([rng.choice(special, 2, replace=False), rng.choice(pool, 6)]))
            rng.shuffle(w)
            out.append((w[:SCAN_STRIDE], rng.choice([1000, 50000, 2000000], min(len(w), SCAN_STRIDE))))
        return out

    case = Case(nwords, SCAN_STRIDE, SCAN_CAP)
    kw, kv = rows(draw(40), SCAN_STRIDE)
    qw, qv = rows(draw(7) + [([], [])], SCAN_STRIDE)
    case.add(kw[:25], kv[:25])
    case.notes["first"] = case.query(qw, qv, 16, 0, None, ("scan", nwords, "25 key frames"))
    case.add(kw[25:], kv[25:])
    case.query(qw, qv, 16, 80, None, ("scan", nwords, "pct 80"))
    case.query(qw, qv, 4, 0, rng.integers(0, 42, len(qw)), ("scan", nwords, "limits"))
    case.notes.update(special=special, kw=kw, qw=qw)
    _TABLE.clear()                                                    # (128 MB at 2^24 words)
    return case


# counts on add and query
@functools.lru_cache(maxsize=None)
def counts_case():
    """Every row is full of words of one small pool, so a slot past the count would match if it were read."""
    rng = np.random.default_rng(26)
    S, nwords = 8, 100
    pool = rng.choice(nwords, 12, replace=False)

    def full_rows(count):
        return (np.stack([rng.choice(pool, S, replace=False) for _ in range(count)]).astype(np.int64),
                rng.choice([1000, 50000, 2000000], (count, S)))

    def cut(word, val, counts):
        keep = np.arange(S)[None, :] < np.array([clamp_count(c, S) for c in counts])[:, None]
        return np.where(keep, word, -1), np.where(keep, val, 0)

    add_n, q_n = [0, COUNT_INVALID, S, S + 5, 1, 3, S], [0, COUNT_INVALID, S, S + 5, 1, 5]
    kw, kv = full_rows(len(add_n))
    qw, qv = full_rows(len(q_n))
    case, blind = Case(nwords, S, 16), Case(nwords, S, 16)          # blind: what reading every slot would give
    case.add(*cut(kw, kv, add_n), gpu=gpu_rows(kw, kv, add_n))
    blind.add(kw, kv)
    for topk, pct in ((8, 0), (3, 80)):
        case.query(*cut(qw, qv, q_n), topk, pct, None, ("counts", topk, pct), gpu=gpu_rows(qw, qv, q_n))
        blind.query(qw, qv, topk, pct, None)
    case.notes.update(blind=blind, add_n=add_n, q_n=q_n)
    return case


# weights
W_STRIDE, W_NWORDS = 16384, 20000
M64 = (1 << 64) - 1


def ref_weights_mod64(word, tf, idf, nwords):
    """The header's formula with its arithmetic modulo 2^64, in Python integers."""
    a = [int(t) * (0 if int(w) >= nwords else 1 if idf is None else min(int(idf[int(w)]), 65535)) for w, t in zip(word, tf)]
    A = sum(a) & M64
    return [0 if A == 0 else ((x << 24) & M64) // A for x in a], a


@functools.lru_cache(maxsize=None)
def weights_case():
    """Rows at stride 16384; every slot holds a word and a tf, so a slot past n would be written if it were read."""
    rng = np.random.default_rng(27)
    ns = [1, 1024, 1025, W_STRIDE, 0, 1025, 1024, W_STRIDE + 5, COUNT_INVALID]
    B = len(ns)
    word = np.stack([rng.choice(W_NWORDS + 1000, W_STRIDE, replace=False) for _ in range(B)]).astype(np.uint32)
    tf = rng.integers(1, 5, (B, W_STRIDE)).astype(np.uint32)
    word[3] = rng.choice(W_NWORDS, W_STRIDE, replace=False)          # the contract limit: tf sums to 16384, every word known
    tf[3] = 1
    tf[5] = rng.integers(0, 1 << 32, W_STRIDE, dtype=np.uint64).astype(np.uint32)     # outside the contract
    tf[5, [0, 7, 1024]] = 0xFFFFFFFF
    word[5, [0, 7, 1024]] = [3, 4, 5]
    word[6] = W_NWORDS + rng.choice(50000, W_STRIDE, replace=False)   # A == 0: no word below nwords
    idf = rng.integers(0, 200000, W_NWORDS).astype(np.uint32)
    idf[rng.random(W_NWORDS) < 0.1] = 0
    idf[[3, 4, 5]] = [65535, 70000, 65534]
    top = rng.choice([65535, 100000], W_NWORDS).astype(np.uint32)     # idf 65535 for every word
    tables = {"idf": idf, "idf 65535": top, "null": None}
    expect, wraps = {}, 0
    for name, table in tables.items():
        rows_ = []
        for b, n_in in enumerate(ns):
            n = clamp_count(n_in, W_STRIDE)
            e, a = ref_weights_mod64(word[b, :n], tf[b, :n], table, W_NWORDS)
            assert all(x < 1 << 32 for x in e)                        # (the formula's value fits the 32-bit output)
            if b == 5:
                wraps += sum((x << 24) > M64 for x in a)
            rows_.append(np.array(e, np.uint32))
        expect[name] = rows_
    return dict(ns=ns, word=word, tf=tf, tables=tables, expect=expect, wraps=wraps)


# ---- CPU: the cases reach what they are meant to reach ---------------------------------------------------------------
def _ties_across(ids, scores, div):
    live = [(s, i // div) for i, s in zip(ids, scores) if i >= 0]
    return any(s1 == s2 and d1 != d2 for k, (s1, d1) in enumerate(live) for s2, d2 in live[k + 1:])


def test_limit_cases_exercise_what_they_claim():
    # the plan, restated from the header
    assert plan(49152) == (2, 24576, 6) and plan(24577) == (2, 12290, 4) and plan(12000) == (1, 12000, 2)
    assert plan(1 << 20)[2] * 64 == 8192 and plan(70000) == (3, 23334, 9) and 6 * ACC_MAX_SLICE == 147456
    # growth: ids on both sides of every boundary below the size, a tie across selection slices, and the dword pairs
    for capacity in (49152, 24577):
        case = growth_case(capacity)
        _, _, sizes, bounds, one, full = growth_frames(capacity)
        sl = case.notes["slice"]
        assert sl in bounds and SEL_SLICE in bounds and len(one) + len(full) <= GROW_TOPK
        assert (capacity + 1) // 2 * 2 - capacity == capacity % 2 and capacity in sizes
        for size, (ids, sc, cm, mx) in case.notes["all_rows"]:
            got = dict(zip(ids, cm))
            for b in [b for b in bounds if b < size]:
                assert {b - 2, b - 1} & set(got) and {b, b + 1} & set(got), (capacity, size, b, ids)
                if b in got and b + 1 in got:
                    assert (got[b], got[b + 1]) == (1, GROW_STRIDE)
                if b - 1 in got:
                    assert got[b - 1] == GROW_STRIDE
            assert mx == GROW_STRIDE and (size - 1 in got or size - 1 in one or size - 2 in got)
            if size >= sl - 1:
                assert _ties_across(ids, sc, SEL_SLICE), (capacity, size)
        last = dict(zip(*case.notes["all_rows"][-1][1][0:3:2]))
        assert any(b in last and b + 1 in last for b in bounds)
    # long lists: from the lengths alone
    case = long_case()
    lens, queries = case.notes["lens"], case.notes["queries"]
    assert sorted(set(lens.tolist())) == [1, 1023, 1024, 1025, 1100] and (lens >= 1025).sum() >= 2100
    assert sorted(int((lens[q] > LONG).sum()) for q in queries) == [40, QUEUE, QUEUE + 1, QUEUE + 1, 2100]
    assert set(lens[queries[2]].tolist()) == {1024, 1025}
    assert any((lens[q] <= LONG).any() and (lens[q] > LONG).sum() > QUEUE for q in queries)
    posted = np.bincount(case.ref.word[case.ref.word >= 0], minlength=LONG_WORDS)
    assert (posted == lens).all() and (case.ref.word[0] >= 0).all() and case.ref.size == LONG_CAP
    assert int(case.ref.val.sum(1).max()) <= Q24
    # merge: slice 127 and slice 0 in one top 64, ties, more candidates than 64, every register row of the merge
    case = merge_case()
    assert case.ref.size == MERGE_SIZE > 127 * SEL_SLICE and plan(case.ref.capacity)[2] == 128
    for key in ("first", "after"):
        exp, ncand = case.notes[key]
        ids, sc = exp[0][0], exp[0][1]
        slices = {i // SEL_SLICE for i in ids if i >= 0}
        assert {0, 127} <= slices and ncand[0] > 64 and len(set(sc)) < len(sc), (key, slices, ncand)
        if key == "first":
            assert {s * 64 // 1024 for s in slices} == set(range(8))      # partial key sel * 64 + k sits in row (sel * 64) / 1024
            assert min(ncand[:3]) > 64 and not (set(range(1, 16)) & slices)
    assert len(case.notes["dead"]) >= 1000 and set(case.notes["dead"]) & set(case.notes["first"][0][0][0])
    # scan: the edge words are indexed, found, and the chunk counts are the intended ones
    for nwords, chunks in ((16384, 1), (16385, 2), (1 << 24, 1024)):
        case = scan_case(nwords)
        assert -(-nwords // SCAN_CHUNK) == chunks
        kw, qw = case.notes["kw"], case.notes["qw"]
        for w in case.notes["special"]:
            assert ((kw == w).any() and (qw == w).any()) and (w < nwords or w == 16384 == nwords)
        assert (kw >= nwords).any() and (qw >= nwords).any() and nwords - 1 in case.notes["special"]
        exp, ncand = case.notes["first"]
        assert sum(n > 0 for n in ncand) >= 7 and ncand[-1] == 0
    # counts: reading a slot past the count would change the result
    case = counts_case()
    for a, b in zip([s for s in case.steps if s[0] == "query"], [s for s in case.notes["blind"].steps if s[0] == "query"]):
        differ = [x != y for x, y in zip(a[5], b[5])]
        assert differ[0] and differ[1] and differ[4], differ           # (the queries of count 0, invalid and 1 at least)
    # weights: the in-contract rows are what ref_weights gives, the limit row is at the limit, the other one wraps
    wc = weights_case()
    for name, table in wc["tables"].items():
        for b, n_in in enumerate(wc["ns"]):
            n = clamp_count(n_in, W_STRIDE)
            if b != 5 and b % 3 == 0:
                assert (wc["expect"][name][b] == ref_weights(wc["word"][b, :n], wc["tf"][b, :n], table, W_NWORDS)).all()
    assert int(wc["tf"][3].sum()) == 16384 and (wc["tables"]["idf 65535"] >= 65535).all() and (wc["word"][3] < W_NWORDS).all()
    assert wc["wraps"] >= 100 and all(not e[6].any() for e in wc["expect"].values()) and wc["expect"]["null"][6].size == 1024
    assert (wc["word"][:3] >= W_NWORDS).any() and int(wc["tf"][5].max()) == 0xFFFFFFFF


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("capacity", [49152, 24577])
def test_gpu_growth_across_slice_boundaries(gpu_ctx, capacity):
    """49152: two accumulate slices of 24576 ids, the 147456-byte LDS launch.  24577: odd, cap_pad 24578, slices of 12290,
    a fourth selection slice of one id.  Grown through 8191, 8192, 8193, slice - 1, slice, slice + 1, capacity - 1 and
    capacity, queried at each size."""
    run_case(gpu_ctx, growth_case(capacity))


@pytest.mark.gpu
def test_gpu_long_lists_fill_and_pass_the_queue(gpu_ctx):
    """Queries with exactly 2048, 2049 and 2100 posting lists longer than 1024 (the queue holds 2048: the others are
    walked in place), and one with lists of 1024 and 1025 only."""
    run_case(gpu_ctx, long_case())


@pytest.mark.gpu
def test_gpu_full_merge_at_capacity_2_pow_20(gpu_ctx):
    """128 selection slices x topk 64 = 8192 partial keys: the merge is exactly full, eight keys per thread."""
    run_case(gpu_ctx, merge_case())


@pytest.mark.gpu
@pytest.mark.parametrize("nwords", [16384, 16385, 1 << 24])
def test_gpu_scan_chunk_edges(gpu_ctx, nwords):
    """One full chunk, one chunk and one word, and 1024 chunks (one chunk sum per thread of k_db_scan_sums)."""
    run_case(gpu_ctx, scan_case(nwords))


@pytest.mark.gpu
def test_gpu_counts_on_add_and_query(gpu_ctx):
    run_case(gpu_ctx, counts_case())


@pytest.mark.gpu
def test_gpu_weights_at_stride_16384_and_modulo_2_pow_64(gpu_ctx):
    import torch
    from pislam_amd.frontend import bowWeightBatch
    wc = weights_case()
    d_word, d_tf, d_n = T(wc["word"]), T(wc["tf"]), T(np.array(wc["ns"], np.uint32))
    for name, table in wc["tables"].items():
        out = filled(wc["word"].shape)
        bowWeightBatch(d_word, d_tf, d_n, None if table is None else T(table), W_NWORDS, out, ctx=gpu_ctx)
        torch.cuda.synchronize()
        got = host(out)
        for b, n_in in enumerate(wc["ns"]):
            n, exp = clamp_count(n_in, W_STRIDE), wc["expect"][name][b]
            assert (got[b, :n] == exp).all(), (name, b, np.flatnonzero(got[b, :n] != exp)[:5])
            assert (got[b, n:] == SENTINEL).all(), ("slot past the count written", name, b)


@pytest.mark.gpu
def test_gpu_inputs_outside_the_contract_stay_inside_the_promise(gpu_ctx):
    """Repeated words and weights of 0xFFFFFFFF on both sides: the values are unspecified; top_id holds -1 or an eligible
    id, no id twice in a row, -1 only at the tail, every row written in full.  The context then serves an in-contract
    query bit for bit."""
    import torch
    from pislam_amd.frontend import BowDatabase
    rng = np.random.default_rng(28)
    nkf, S, nwords, B, topk = 64, 32, 50, 12, 16
    kw = rng.integers(0, 12, (nkf, S)).astype(np.uint32)              # twelve words in 32 slots: repeated
    kw[rng.random((nkf, S)) < 0.1] = 0xFFFFFFFF
    kv = rng.choice([0xFFFFFFFF, 0xFFFFFFFE, 1 << 31, 5], (nkf, S)).astype(np.uint32)
    qw, qv = kw[rng.integers(0, nkf, B)].copy(), rng.choice([0xFFFFFFFF, 1 << 30], (B, S)).astype(np.uint32)
    qw[0] = 3                                                         # one word 32 times
    kn, qn = np.full(nkf, S, np.uint32), rng.choice([S, S + 9, 17], B).astype(np.uint32)
    limits = rng.choice([nkf, nkf + 10, 40, 1, 0, -5], B).astype(np.int32)
    dead = [0, 5, 39, 63]
    db = BowDatabase(nwords, S, nkf, ctx=gpu_ctx)
    assert db.add(T(kw), T(kv), T(kn)) == 0
    db.remove(dead)
    for lim in (None, limits):
        for pct in (0, 80):
            runs = []
            for fill in (SENTINEL, 0x3C3C3C3C):
                outs = [filled((B, topk), fill), filled((B, topk), fill), filled((B, topk), fill), filled((B,), fill)]
                db.query(T(qw), T(qv), T(qn), topk=topk, min_common_pct=pct, id_limit=None if lim is None else T(lim),
                         top_id=outs[0], top_score=outs[1], top_common=outs[2], max_common=outs[3])
                torch.cuda.synchronize()
                runs.append([host(o) for o in outs])
            for a, b in zip(*runs):
                assert (a == b).all(), "an output element was not written (it kept the fill it had)"
            ids = runs[0][0].view(np.int32)
            for b in range(B):
                row, bound = ids[b].tolist(), nkf if lim is None else min(nkf, int(lim[b]))
                live = [i for i in row if i != -1]
                assert all(0 <= i < bound and i not in dead for i in live), (b, row, bound)
                assert len(set(live)) == len(live) and row == live + [-1] * (topk - len(live)), (b, row)
                assert all(runs[0][1][b, k] == 0 and runs[0][2][b, k] == 0 for k in range(len(live), topk))
    db.close()
    run_case(gpu_ctx, counts_case())                                  # the context is as good as before


@pytest.mark.gpu
def test_gpu_two_databases_share_a_context_and_a_captured_query(gpu_ctx):
    """A (capacity 49152, 147456 bytes of LDS) and B (capacity 12000, 72000 bytes) on one context: eager A, B, A; then a
    query of A captured on a side stream (one stream, no parallel branches, after reserve_query), replayed, an eager
    query of B, A grown outside the graph from slice - 1 to slice + 1 key frames, and the replay again."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import BowDatabase
    word, val, _, _, _, _ = growth_frames(49152)
    sl, S, topk = plan(49152)[1], GROW_STRIDE, 16
    assert plan(12000)[1] * 6 == 72000 and sl * 6 == 147456
    ref_a, ref_b = DenseDb(GROW_WORDS, S, 49152), DenseDb(GROW_WORDS, S, 12000)
    qa = rows([([3, 0, 2, 1], [Q24 // 4] * 4), (word[sl - 3], [2500] * 4), (word[70], [2500] * 4), ([0, 2], [Q24 // 4, 9])], S)
    qb = rows([([3, 0, 2, 1], [Q24 // 4] * 4), (word[9000], [2500] * 4), ([], [])], S)

    def expect(ref, q, pct):
        return [list(ref_query_fast(ref, q[0][b][q[0][b] >= 0], q[1][b][q[0][b] >= 0], None, pct, topk, want_all=False)[:4])
                for b in range(len(q[0]))]

    side = torch.cuda.Stream(dev())
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        a, b = BowDatabase(GROW_WORDS, S, 49152, ctx=ctx), BowDatabase(GROW_WORDS, S, 12000, ctx=ctx)
        assert a.add(*[T(x) for x in gpu_rows(word[:sl - 1], val[:sl - 1])]) == ref_a.add(word[:sl - 1], val[:sl - 1]) == 0
        assert b.add(*[T(x) for x in gpu_rows(word[8000:11000], val[8000:11000])]) == ref_b.add(word[8000:11000], val[8000:11000]) == 0
        for db, ref, q, what in ((a, ref_a, qa, "A"), (b, ref_b, qb, "B"), (a, ref_a, qa, "A after B")):
            for pct in (0, 80):
                compare(gpu_query_arrays(db, gpu_rows(*q), topk, pct, None), expect(ref, q, pct), ("eager", what, pct))
        a.reserve_query(len(qa[0]), topk)
        d_q = [T(x) for x in gpu_rows(*qa)]
        outs = [filled((len(qa[0]), topk)), filled((len(qa[0]), topk)), filled((len(qa[0]), topk)), filled((len(qa[0]),))]
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            a.query(*d_q, topk=topk, min_common_pct=0, top_id=outs[0], top_score=outs[1], top_common=outs[2], max_common=outs[3])
        g.replay()
        side.synchronize()
        compare([host(o) for o in outs], expect(ref_a, qa, 0), "first replay")
        compare(gpu_query_arrays(b, gpu_rows(*qb), topk, 0, None), expect(ref_b, qb, 0), "eager B between the replays")
        assert a.add(*[T(x) for x in gpu_rows(word[sl - 1:sl + 1], val[sl - 1:sl + 1])]) == ref_a.add(word[sl - 1:sl + 1], val[sl - 1:sl + 1])
        assert a.size == sl + 1
        for o in outs:
            o.fill_(7)
        g.replay()
        side.synchronize()
        exp = expect(ref_a, qa, 0)
        compare([host(o) for o in outs], exp, "second replay, A grown across the slice start")
        assert sl in exp[0][0] and sl - 1 in exp[0][0]                # the new key frames are among the best
        compare(gpu_query_arrays(a, gpu_rows(*qa), topk, 80, None), expect(ref_a, qa, 80), "eager A at the end")
        a.close(), b.close()
