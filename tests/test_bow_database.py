"""Key-frame database for bag-of-words place recognition: pislam_bow_weight_batch (Q24 integer tf-idf weights) and
pislam_bowdb_* (forward store, inverted file, scored top-k query) against a NumPy / Python-integer statement of their
semantics that is independent of the library (include/pislam_hip.h): weights by the formula in
Python integers, `common` and `score` by an explicit join of the two entry lists (no inverted file), the selection by
sorted(candidates, key=(-score, id)).  Every result is an integer; the GPU results are compared bit for bit."""
import numpy as np
import pytest

from test_bow import (COUNT_INVALID, STRIDE, T, dev, fe_descriptors, filled, host, make_vocab, run_transform, run_vector,
                      transform_inputs)
from test_match_window import SENTINEL, clamp_count

Q24 = 1 << 24


# ---- the reference -----------------------------------------------------------------------------------------------------
def ref_weights(word, tf, idf, nwords):
    """Q24 weights of one frame's entries (Python integers)."""
    a = [int(t) * (0 if int(w) >= nwords else 1 if idf is None else min(int(idf[int(w)]), 65535)) for w, t in zip(word, tf)]
    A = sum(a)
    return np.array([0 if A == 0 else (x << 24) // A for x in a], np.uint32)


class RefDb:
    """Key frames as plain entry lists; ids in order of addition."""

    def __init__(self, nwords, stride, capacity):
        self.nwords, self.stride, self.capacity = nwords, stride, capacity
        self.frames, self.alive = [], []

    def add(self, frames):
        if len(self.frames) + len(frames) > self.capacity:
            raise ValueError("capacity")
        first = len(self.frames)
        for w, v in frames:
            self.frames.append((np.asarray(w[:self.stride], np.int64), np.asarray(v[:self.stride], np.int64)))
            self.alive.append(True)
        return first

    def remove(self, ids):
        ids = [int(i) for i in ids]
        if len(set(ids)) != len(ids) or any(i < 0 or i >= len(self.frames) or not self.alive[i] for i in ids):
            raise ValueError("id")
        for i in ids:
            self.alive[i] = False

    def clear(self):
        self.frames, self.alive = [], []


def ref_pair(qw, qv, kw, kv, nwords):
    """(common, score) of two entry lists with distinct words: the explicit join."""
    qw, kw = np.asarray(qw, np.int64), np.asarray(kw, np.int64)
    _, qi, ki = np.intersect1d(qw, kw, return_indices=True)
    keep = qw[qi] < nwords
    qi, ki = qi[keep], ki[keep]
    return len(qi), int(np.minimum(np.asarray(qv, np.int64)[qi], np.asarray(kv, np.int64)[ki]).sum())


def ref_query(db, qw, qv, limit=None, pct=80, topk=16):
    """One query: (top_id, top_score, top_common lists of topk, max_common, number of candidates, all (id, common,
    score) of the eligible key frames)."""
    elig = [k for k in range(len(db.frames)) if db.alive[k] and (limit is None or k < limit)]
    cs = {k: ref_pair(qw, qv, *db.frames[k], db.nwords) for k in elig}
    max_common = max([c for c, _ in cs.values()], default=0)
    cand = [k for k in elig if cs[k][0] >= 1 and cs[k][0] * 100 >= pct * max_common]
    order = sorted(cand, key=lambda k: (-cs[k][1], k))[:topk]
    pad = topk - len(order)
    return ([*order, *[-1] * pad], [*[cs[k][1] for k in order], *[0] * pad], [*[cs[k][0] for k in order], *[0] * pad],
            max_common, len(cand), cs)


def frame(words, weights):
    return np.asarray(words, np.int64), np.asarray(weights, np.int64)


# ---- CPU: the reference itself ---------------------------------------------------------------------------------------
def test_reference_hand_built_cases():
    db = RefDb(100, 8, 16)
    db.add([frame([1, 2, 3], [10, 20, 30]),        # 0
            frame([1, 2, 3], [10, 20, 30]),        # 1: the same vector: a tie, which goes to id 0
            frame([1, 2, 3, 4], [60, 60, 60, 60]), # 2: four common words with the query below, the best score
            frame([7], [5]),                       # 3: nothing in common
            frame([1], [99])])                     # 4: one common word
    q = frame([4, 3, 2, 1], [5, 30, 20, 10])
    ids, sc, cm, mx, ncand, _ = ref_query(db, *q, pct=0, topk=4)
    assert (ids, sc, cm, mx, ncand) == ([2, 0, 1, 4], [65, 60, 60, 10], [4, 3, 3, 1], 4, 4)
    # unsorted entries give what sorted ones give
    assert ref_query(db, *frame([1, 2, 3, 4], [10, 20, 30, 5]), pct=0, topk=4)[:5] == (ids, sc, cm, mx, ncand)
    # min_common_pct: 80 % of 4 = 3.2 keeps only the four-word frame; 75 would keep the three-word ones; 100 likewise
    assert ref_query(db, *q, pct=80, topk=4)[:5] == ([2, -1, -1, -1], [65, 0, 0, 0], [4, 0, 0, 0], 4, 1)
    assert ref_query(db, *q, pct=75, topk=4)[0] == [2, 0, 1, -1]
    assert ref_query(db, *q, pct=100, topk=2)[:3] == ([2, -1], [65, 0], [4, 0])
    # a dead and an over-limit key frame are skipped and do not raise max_common
    db.remove([2])
    ids, sc, cm, mx, ncand, _ = ref_query(db, *q, pct=80, topk=3)
    assert (ids, sc, cm, mx, ncand) == ([0, 1, -1], [60, 60, 0], [3, 3, 0], 3, 2)
    assert ref_query(db, *q, limit=1, pct=80, topk=3)[:4] == ([0, -1, -1], [60, 0, 0], [3, 0, 0], 3)
    assert ref_query(db, *q, limit=0, pct=80, topk=2)[:5] == ([-1, -1], [0, 0], [0, 0], 0, 0)
    assert ref_query(db, *q, limit=-3, pct=0, topk=1)[:5] == ([-1], [0], [0], 0, 0)
    with pytest.raises(ValueError):
        db.remove([2])
    with pytest.raises(ValueError):
        db.remove([5])
    # a word at or above nwords is not indexed and not counted
    db2 = RefDb(4, 8, 4)
    db2.add([frame([1, 4, 9], [1, 2, 3])])
    assert ref_query(db2, *frame([9, 4, 1], [7, 7, 7]), pct=0, topk=1)[:4] == ([0], [1], [1], 1)
    # an entry list longer than the database's stride keeps its first entries
    db3 = RefDb(100, 2, 4)
    db3.add([frame([5, 6, 7], [1, 1, 1])])
    assert ref_query(db3, *frame([7, 6], [9, 9]), pct=0, topk=1)[:3] == ([0], [1], [1])


def test_reference_weights():
    w = ref_weights([3, 5, 9], [1, 2, 1], None, 10)
    assert w.tolist() == [Q24 // 4, Q24 // 2, Q24 // 4]
    assert ref_weights([3, 5, 9], [1, 2, 1], None, 6).tolist() == [(1 << 24) // 3, (2 << 24) // 3, 0]   # word 9 >= nwords
    idf = np.zeros(10, np.uint32)
    assert ref_weights([3, 5, 9], [1, 2, 1], idf, 10).tolist() == [0, 0, 0]                               # all-zero idf
    idf[3], idf[5] = 1 << 20, 65535                                                                       # above 65535 counts as 65535
    assert ref_weights([3, 5], [1, 1], idf, 10).tolist() == [Q24 // 2, Q24 // 2]
    w = ref_weights(np.arange(1000), np.full(1000, 3), np.arange(1000) % 7, 1000)
    assert int(w.astype(np.int64).sum()) <= Q24 and int(w.astype(np.int64).sum()) > Q24 - 1000
    # zero weights on both sides: common counts, the score is 0, the frame is still a candidate
    db = RefDb(10, 4, 2)
    db.add([frame([3, 5], [0, 0])])
    assert ref_query(db, *frame([3, 5], [0, 0]), pct=80, topk=2)[:4] == ([0, -1], [0, 0], [2, 0], 2)


def test_integer_score_against_the_float_l1_score():
    """score / 2^24 against DBoW2's L1 score of the same tf-idf vectors in float64: every floored weight is less than
    one unit of 2^-24 below its exact value and min keeps that, so for c common words
    0 <= s_float - score / 2^24 < c * 2^-24 (1e-9 for the float sums)."""
    rng = np.random.default_rng(5)
    nwords, checked = 5000, 0
    for _ in range(200):
        idf = rng.integers(0, 70000, nwords)
        idf[rng.random(nwords) < 0.05] = 0
        vecs = []
        for _ in range(2):
            w = rng.choice(nwords, int(rng.integers(1, 600)), replace=False)
            tf = rng.integers(1, 6, len(w))
            vecs.append((w, tf))
        if rng.random() < 0.5:                                       # share many words
            k = min(len(vecs[0][0]), len(vecs[1][0])) // 2
            w1 = vecs[1][0].copy()
            w1[:k] = vecs[0][0][:k]
            if len(np.unique(w1)) == len(w1):
                vecs[1] = (w1, vecs[1][1])
        ints, flts = [], []
        for w, tf in vecs:
            ints.append(ref_weights(w, tf, idf, nwords))
            a = tf.astype(np.float64) * np.minimum(idf[w], 65535)
            flts.append(a / a.sum() if a.sum() > 0 else a)
        c, score = ref_pair(vecs[0][0], ints[0], vecs[1][0], ints[1], nwords)
        dense = np.zeros((2, nwords))
        for d, (w, _), f in zip(dense, vecs, flts):
            d[w] = f
        s_min = float(np.minimum(dense[0], dense[1]).sum())
        if dense[0].sum() > 0 and dense[1].sum() > 0:
            assert abs(s_min - (1.0 - 0.5 * np.abs(dense[0] - dense[1]).sum())) < 1e-9     # the two forms of the L1 score
            checked += 1
        diff = s_min - score / Q24
        assert -1e-9 <= diff < c / Q24 + 1e-9, (diff, c)
    assert checked >= 150


def test_python_side_checks_need_no_device():
    """BowDatabase and bowWeightBatch refuse bad shapes and ranges before they touch the library."""
    from pislam_amd.frontend import BowDatabase, bowWeightBatch
    for nwords, stride, capacity in [(0, 16, 10), ((1 << 24) + 1, 16, 10), (100, 0, 10), (100, 16385, 10), (100, 16, 0),
                                     (100, 16, (1 << 20) + 1), (100, 16384, 1 << 20)]:
        with pytest.raises(ValueError):
            BowDatabase(nwords, stride, capacity)
    w, n = np.zeros((2, 16), np.int32), np.zeros(2, np.int32)
    idf = np.ones(100, np.int32)
    for args in [(w[0], w[0], n), (w, w[:, :8], n), (w, w, n[:1]), (w, w, n, idf.reshape(10, 10)), (w, w, n, None, None),
                 (w, w, n, idf, 101), (w, w, n, None, 0), (np.zeros((2, 16385), np.int32),) * 2 + (n,)]:
        with pytest.raises(ValueError):
            bowWeightBatch(*args)
    with pytest.raises(ValueError):
        bowWeightBatch(w, w, n, idf, 100, np.zeros((2, 8), np.int32))
    db = BowDatabase.__new__(BowDatabase)                            # the argument checks come before any use of the handle
    db.h = None
    for call in [lambda: db.add(w, w[:, :8], n), lambda: db.add(w, w, n[:1]), lambda: db.query(w, w, n, topk=0),
                 lambda: db.query(w, w, n, topk=65), lambda: db.query(w, w, n, min_common_pct=-1),
                 lambda: db.query(w, w, n, min_common_pct=101), lambda: db.query(w, w, n, id_limit=np.zeros(3, np.int32)),
                 lambda: db.query(w, w, n, topk=4, top_id=np.zeros((2, 5), np.int32)), lambda: db.reserve_query(1, 65),
                 lambda: db.reserve_query(-1, 4)]:
        with pytest.raises(ValueError):
            call()


# ---- GPU helpers -----------------------------------------------------------------------------------------------------
def pack(frames, stride, counts=None):
    """[B][stride] word / weight arrays (SENTINEL past the entries) and the counts of a list of entry lists."""
    B = len(frames)
    word = np.full((B, stride), SENTINEL, np.uint32)
    val = np.full((B, stride), SENTINEL, np.uint32)
    n = np.zeros(B, np.uint32)
    for b, (w, v) in enumerate(frames):
        k = min(len(w), stride)
        word[b, :k], val[b, :k], n[b] = np.asarray(w[:k], np.uint32), np.asarray(v[:k], np.uint32), len(w)
    if counts is not None:
        n = np.asarray(counts, np.uint32)
    return word, val, n


def gpu_add(db, frames, stride):
    word, val, n = pack(frames, stride)
    return db.add(T(word), T(val), T(n))


def gpu_query(db, frames, stride, topk, pct, limit=None):
    import torch
    word, val, n = pack(frames, stride)
    B = len(frames)
    outs = [filled((B, topk)), filled((B, topk)), filled((B, topk)), filled((B,))]
    lim = None if limit is None else T(np.asarray(limit, np.int32))
    db.query(T(word), T(val), T(n), topk=topk, min_common_pct=pct, id_limit=lim, top_id=outs[0], top_score=outs[1],
             top_common=outs[2], max_common=outs[3])
    torch.cuda.synchronize()
    return [host(o) for o in outs]


def check_query(got, ref_db, frames, stride, topk, pct, limit=None, what=""):
    """Bit for bit against the reference; returns per query (number of candidates, whether the top k holds a tie)."""
    info = []
    for b, (w, v) in enumerate(frames):
        lim = None if limit is None else int(limit[b])
        ids, sc, cm, mx, ncand, _ = ref_query(ref_db, w[:stride], v[:stride], lim, pct, topk)
        g = [got[0][b].view(np.int32).tolist(), got[1][b].tolist(), got[2][b].tolist(), int(got[3][b])]
        assert g == [ids, sc, cm, mx], (what, b, g, [ids, sc, cm, mx])
        live = [s for i, s in zip(ids, sc) if i >= 0]
        info.append((ncand, len(set(live)) < len(live)))
    return info


def place_frames(rng, nwords, nplaces, per_place, place_words, frame_words, noise, idf, sets=None):
    """Synthetic vectors with place structure: a place is a seeded word set; a frame of it holds a random part of the
    set plus noise words, with random tf and the Q24 weights of `idf`.  Returns (frames, place of each frame, sets)."""
    if sets is None:
        sets = [rng.choice(nwords, min(place_words, nwords), replace=False) for _ in range(nplaces)]
    frames, place = [], []
    for p in range(nplaces):
        for _ in range(per_place):
            own = rng.choice(sets[p], min(frame_words, len(sets[p])), replace=False)
            w = np.unique(np.concatenate([own, rng.integers(0, nwords, noise)]))
            rng.shuffle(w)                                           # entries need not be sorted
            tf = rng.integers(1, 5, len(w))
            frames.append(frame(w, ref_weights(w, tf, idf, nwords)))
            place.append(p)
    return frames, place, sets


# ---- GPU: weights ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,words", [("b3", 8), ("a", 1), ("b4", 4)])
def test_gpu_weights_on_vector_outputs(gpu_ctx, kind, words):
    import torch
    from pislam_amd.frontend import bowWeightBatch
    vocab, tree = make_vocab(gpu_ctx, kind, words, 2)
    desc, counts = transform_inputs(words, 7)                       # counts 0, PISLAM_COUNT_INVALID and above the stride included
    word = run_transform(gpu_ctx, vocab, desc, counts)[0]
    bw, tf, bn = run_vector(gpu_ctx, word, counts)
    nwords = tree["nwords"]
    rng = np.random.default_rng([3, words])
    idf = rng.integers(0, 200000, nwords).astype(np.uint32)
    idf[rng.random(nwords) < 0.1] = 0
    assert (idf == 0).any() and (idf > 65535).any()
    # the counts the weight call reads: the vector's own, then one 0, one invalid and one above the stride
    for n_in in (bn, np.array([bn[0], 0, COUNT_INVALID, STRIDE + 5, bn[4], bn[5]], np.uint32)):
        for table, nw in ((idf, nwords), (None, nwords), (idf, max(1, nwords // 2))):
            out = filled(bw.shape)
            bowWeightBatch(T(bw), T(tf), T(n_in), None if table is None else T(table), nw, out, ctx=gpu_ctx)
            torch.cuda.synchronize()
            got = host(out)
            for b in range(len(n_in)):
                n = clamp_count(n_in[b], bw.shape[1])
                exp = ref_weights(bw[b, :n], tf[b, :n], table, nw)
                assert (got[b, :n] == exp).all(), (kind, b, np.flatnonzero(got[b, :n] != exp)[:5])
                assert (got[b, n:] == SENTINEL).all(), ("slot past the count written", b)
    vocab.close()


# ---- GPU: add + query on synthetic place vectors ---------------------------------------------------------------------
def places_case(nwords, nkf, nplaces, place_words, frame_words, noise, seed, nq):
    """Key frames with place structure (some stored twice, so that scores tie), queries (new frames of the places, a
    stored vector itself, an empty one), the place of each, and the id_limit forms."""
    rng = np.random.default_rng(seed)
    idf = rng.integers(1, 3000, nwords)
    frames, place, sets = place_frames(rng, nwords, nplaces, -(-nkf // nplaces), place_words, frame_words, noise, idf)
    frames, place = frames[:nkf], place[:nkf]
    for k in rng.choice(nkf // 2, max(1, nkf // 10), replace=False):     # twice: a tie that goes to the smaller id
        frames[nkf - 1 - int(k)] = frames[int(k)]
        place[nkf - 1 - int(k)] = place[int(k)]
    qfr, qplace, _ = place_frames(rng, nwords, nplaces, 1, place_words, frame_words, noise, idf, sets)
    pick = rng.choice(len(qfr), min(nq, len(qfr)), replace=False)
    queries = [qfr[i] for i in pick] + [frames[0], frame([], [])]
    B = len(queries)
    limits = {"null": None, "random": rng.integers(1, nkf + 2, B), "none": np.array([0, -5] * B)[:B]}
    return rng, frames, place, queries, [qplace[i] for i in pick], limits


def run_places(gpu_ctx, nwords, nkf, capacity, stride, topk, nplaces, place_words, frame_words, noise, seed, nq=20):
    """Database of `nkf` place frames queried under every id_limit form and min_common_pct 0 / 80 / 100; then removed
    ids; then clear and re-add."""
    from pislam_amd.frontend import BowDatabase
    rng, frames, place, queries, qplace, limits = places_case(nwords, nkf, nplaces, place_words, frame_words, noise, seed, nq)
    pick = qplace
    ref = RefDb(nwords, stride, capacity)
    db = BowDatabase(nwords, stride, capacity, ctx=gpu_ctx)
    assert db.add(*[T(a) for a in pack(frames, stride)]) == ref.add(frames) == 0 and db.size == nkf
    ties = fewer = more = filtered = place_hits = 0
    for pct in (80, 0, 100):
        for name, lim in limits.items():
            got = gpu_query(db, queries, stride, topk, pct, lim)
            info = check_query(got, ref, queries, stride, topk, pct, lim, what=(pct, name))
            if name != "none":
                ties += sum(t for _, t in info)
                fewer += sum(n < topk for n, _ in info)
                more += sum(n > topk for n, _ in info)
            if name == "null" and pct == 80:
                for b in range(len(pick)):
                    cs = ref_query(ref, *queries[b], None, pct, topk)[5]
                    filtered += any(c >= 1 and c * 100 < 80 * int(got[3][b]) for c, _ in cs.values())
                    place_hits += int(got[0][b, 0]) < nkf and place[int(got[0][b, 0])] == qplace[b]
    print(f"nwords {nwords} key frames {nkf} topk {topk}: ties in a top k {ties}, queries with fewer / more candidates "
          f"than topk {fewer} / {more}, 80 % filter excluded someone for {filtered} of {len(pick)}, best is of the "
          f"query's place {place_hits} of {len(pick)}")
    # removed ids
    dead = sorted({int(i) for i in rng.choice(nkf, max(1, nkf // 8), replace=False)} | {0})
    db.remove(dead), ref.remove(dead)
    for name in ("null", "random"):
        check_query(gpu_query(db, queries, stride, topk, 80, limits[name]), ref, queries, stride, topk, 80, limits[name],
                    what=("removed", name))
    # clear, then re-add in another order: ids restart at 0
    db.clear(), ref.clear()
    assert db.size == 0
    check_query(gpu_query(db, queries, stride, topk, 80), ref, queries, stride, topk, 80, what="cleared")
    again = frames[::-1][:max(1, nkf // 2)]
    assert gpu_add(db, again, stride) == ref.add(again) == 0
    check_query(gpu_query(db, queries, stride, topk, 80), ref, queries, stride, topk, 80, what="re-added")
    db.close()
    return ties, fewer, more


@pytest.mark.gpu
def test_gpu_query_places_300_key_frames_1000_words(gpu_ctx):
    ties, fewer, more = run_places(gpu_ctx, 1000, 300, 300, 64, 16, nplaces=20, place_words=60, frame_words=40, noise=6, seed=11)
    assert ties >= 1, "no tie inside a reference top k: the tie rule is not tested"
    assert fewer >= 1 and more >= 1, "the reference must see queries with fewer and with more candidates than topk"


@pytest.mark.gpu
def test_gpu_query_places_2000_key_frames_million_words(gpu_ctx):
    ties, fewer, more = run_places(gpu_ctx, 1_000_000, 2000, 2500, 128, 64, nplaces=25, place_words=150, frame_words=100,
                                   noise=10, seed=12, nq=12)
    assert ties >= 1, "no tie inside a reference top k: the tie rule is not tested"
    assert fewer >= 1 and more >= 1, "the reference must see queries with fewer and with more candidates than topk"


@pytest.mark.gpu
def test_gpu_query_topk_1_and_the_smallest_database(gpu_ctx):
    from pislam_amd.frontend import BowDatabase
    run_places(gpu_ctx, 1000, 120, 300, 32, 1, nplaces=10, place_words=40, frame_words=24, noise=4, seed=13, nq=8)
    # one word, one key frame, one entry, one result
    db, ref = BowDatabase(1, 1, 1, ctx=gpu_ctx), RefDb(1, 1, 1)
    queries = [frame([0], [Q24]), frame([0], [5]), frame([1], [Q24]), frame([], [])]
    check_query(gpu_query(db, queries, 1, 1, 80), ref, queries, 1, 1, 80, what="empty")
    assert gpu_add(db, [frame([0], [Q24])], 1) == ref.add([frame([0], [Q24])]) == 0
    for pct in (0, 80, 100):
        check_query(gpu_query(db, queries, 1, 1, pct), ref, queries, 1, 1, pct, what="one")
        check_query(gpu_query(db, queries, 1, 16, pct), ref, queries, 1, 16, pct, what="one, topk 16")
    db.close()


@pytest.mark.gpu
def test_gpu_query_one_word_long_posting_list(gpu_ctx):
    """nwords 1: every key frame holds word 0, one posting list of 3000 (walked by the whole workgroup)."""
    from pislam_amd.frontend import BowDatabase
    rng = np.random.default_rng(14)
    nkf = 3000
    frames = [frame([0], [int(v)]) for v in rng.integers(0, 50, nkf)]        # few distinct weights: many ties
    db, ref = BowDatabase(1, 1, nkf, ctx=gpu_ctx), RefDb(1, 1, nkf)
    assert gpu_add(db, frames, 1) == ref.add(frames) == 0
    queries = [frame([0], [30]), frame([0], [0]), frame([0], [Q24]), frame([3], [7])]
    lim = np.array([nkf, 17, 2999, 5])
    for topk in (1, 16, 64):
        info = check_query(gpu_query(db, queries, 1, topk, 80, lim), ref, queries, 1, topk, 80, lim, what=topk)
        assert topk == 1 or info[0][1], "no tie in the top k"
    db.close()


@pytest.mark.gpu
def test_gpu_query_stride_16384(gpu_ctx):
    from pislam_amd.frontend import BowDatabase
    rng = np.random.default_rng(15)
    nwords, S = 1_000_000, 16384
    idf = rng.integers(1, 3000, nwords)
    base = rng.choice(nwords, 20000, replace=False)
    frames = []
    for n in (S, S, 9000, 1):
        w = rng.choice(base, n, replace=False)
        frames.append(frame(w, ref_weights(w, rng.integers(1, 3, n), idf, nwords)))
    db, ref = BowDatabase(nwords, S, 6, ctx=gpu_ctx), RefDb(nwords, S, 6)
    assert gpu_add(db, frames, S) == ref.add(frames) == 0
    # an add at a smaller stride than the database's
    small = [frame(frames[0][0][:500], frames[0][1][:500])]
    assert gpu_add(db, small, 512) == ref.add(small) == 4
    info = check_query(gpu_query(db, frames, S, 16, 0), ref, frames, S, 16, 0, what="stride 16384")
    assert all(n >= 4 for n, _ in info[:3])                          # (the one-word key frame may share nothing)
    check_query(gpu_query(db, frames, S, 16, 80), ref, frames, S, 16, 80, what="stride 16384, 80 %")
    db.close()
    # a database of a smaller stride than the add's: the first entries are kept
    db, ref = BowDatabase(nwords, 100, 4, ctx=gpu_ctx), RefDb(nwords, 100, 4)
    assert gpu_add(db, frames[:3], S) == ref.add(frames[:3]) == 0
    check_query(gpu_query(db, frames, S, 4, 0), ref, frames, S, 4, 0, what="clamped add")
    db.close()


@pytest.mark.gpu
def test_gpu_query_capacity_70000(gpu_ctx):
    """Three accumulate slices and nine selection slices whose partial lists are merged."""
    from pislam_amd.frontend import BowDatabase
    rng = np.random.default_rng(16)
    nwords, cap, S, nkf = 1000, 70000, 8, 69001
    nq, topk = 6, 16
    print(f"forward store + postings {cap * S * 16 / 1e6:.1f} MB, query workspace {nq * (6 * cap + 4 + 12 * 9 * topk) / 1e6:.1f} MB")
    words = np.stack([rng.choice(nwords, S, replace=False) for _ in range(2000)])
    pick = rng.integers(0, 2000, nkf)                               # 2000 distinct vectors over 69001 ids: ties everywhere
    wts = np.stack([ref_weights(w, rng.integers(1, 4, S), None, nwords) for w in words])
    frames = [frame(words[p], wts[p]) for p in pick]
    db, ref = BowDatabase(nwords, S, cap, ctx=gpu_ctx), RefDb(nwords, S, cap)
    half = 40000
    assert gpu_add(db, frames[:half], S) == ref.add(frames[:half]) == 0
    assert gpu_add(db, frames[half:], S) == ref.add(frames[half:]) == half
    queries = [frames[5], frames[68000], frame(words[7][:5], wts[7][:5]), frame(rng.choice(nwords, S, replace=False), [Q24 // S] * S),
               frames[30000], frame([], [])]
    dead = [int(i) for i in rng.choice(nkf, 500, replace=False)]
    lim = np.array([nkf, 30000, 68500, 70000, 8192, 100])
    info = check_query(gpu_query(db, queries, S, topk, 80), ref, queries, S, topk, 80, what="70000")
    assert any(t for _, t in info) and any(n > topk for n, _ in info)
    db.remove(dead), ref.remove(dead)
    check_query(gpu_query(db, queries, S, topk, 80, lim), ref, queries, S, topk, 80, lim, what="70000, limits, removed")
    check_query(gpu_query(db, queries, S, 64, 0, lim), ref, queries, S, 64, 0, lim, what="70000, topk 64")
    db.close()


@pytest.mark.gpu
def test_gpu_add_in_one_batch_in_several_and_one_by_one(gpu_ctx):
    """The three ways of adding give identical query results; an add past the capacity and a remove of an unknown id
    return the error and the next query is unchanged."""
    from pislam_amd.capi import PislamError
    from pislam_amd.frontend import BowDatabase
    rng = np.random.default_rng(17)
    nwords, S, nkf, topk = 1000, 48, 90, 16
    idf = rng.integers(0, 3000, nwords)
    frames, _, _ = place_frames(rng, nwords, 9, 10, 50, 30, 5, idf)
    queries = frames[::7] + place_frames(rng, nwords, 9, 1, 50, 30, 5, idf)[0]
    ref = RefDb(nwords, S, nkf)
    ref.add(frames)
    results = []
    for cuts in ([0, nkf], [0, 1, 30, 31, 64, nkf], list(range(nkf + 1))):
        db = BowDatabase(nwords, S, nkf, ctx=gpu_ctx)
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert gpu_add(db, frames[a:b], S) == a
        got = gpu_query(db, queries, S, topk, 80)
        check_query(got, ref, queries, S, topk, 80, what=len(cuts))
        results.append(got)
        with pytest.raises(PislamError):
            gpu_add(db, frames[:1], S)                               # the database is full
        for bad in ([nkf], [-1], [3, 3]):
            with pytest.raises(PislamError):
                db.remove(bad)
        assert db.size == nkf
        again = gpu_query(db, queries, S, topk, 80)
        assert all((a == b).all() for a, b in zip(got, again))
        db.remove([3]), ref.remove([3])
        with pytest.raises(PislamError):
            db.remove([3])                                           # already dead
        check_query(gpu_query(db, queries, S, topk, 80), ref, queries, S, topk, 80, what="removed 3")
        ref.alive[3] = True
        db.close()
    for got in results[1:]:
        assert all((a == b).all() for a, b in zip(results[0], got))


# ---- GPU: the front end's outputs ------------------------------------------------------------------------------------
def bow_chain(ctx, vocab, desc, counts, idf, nwords):
    """transform -> vector -> weight on host arrays; returns the vector, the weights and the count, as host arrays."""
    import torch
    from pislam_amd.frontend import bowWeightBatch
    word = run_transform(ctx, vocab, desc, counts)[0]
    bw, tf, bn = run_vector(ctx, word, counts)
    wt = filled(bw.shape)
    bowWeightBatch(T(bw), T(tf), T(bn), T(idf), nwords, wt, ctx=ctx)
    torch.cuda.synchronize()
    return bw, tf, bn, host(wt)


def as_frames(bw, wt, bn):
    return [frame(bw[b, :bn[b]], wt[b, :bn[b]]) for b in range(len(bn))]


@pytest.mark.gpu
def test_gpu_frontend_frames_find_themselves(gpu_ctx):
    from pislam_amd.frontend import BowDatabase
    vocab, tree = make_vocab(gpu_ctx, "b3", 8, 2)
    nwords = tree["nwords"]
    desc, n = fe_descriptors(8)
    idf = np.random.default_rng(18).integers(1, 60000, nwords).astype(np.uint32)
    bw, tf, bn, wt = bow_chain(gpu_ctx, vocab, desc, n.astype(np.uint32), idf, nwords)
    for b in range(len(bn)):
        assert (wt[b, :bn[b]] == ref_weights(bw[b, :bn[b]], tf[b, :bn[b]], idf, nwords)).all()
    frames = as_frames(bw, wt, bn)
    S, B, topk = bw.shape[1], len(bn), 4
    db, ref = BowDatabase(nwords, S, 16, ctx=gpu_ctx), RefDb(nwords, S, 16)
    assert db.add(T(bw), T(wt), T(bn)) == ref.add(frames) == 0
    got = gpu_query(db, frames, S, topk, 80)
    check_query(got, ref, frames, S, topk, 80, what="front end")
    for b in range(B):
        ids, sc, cm, _, _, _ = ref_query(ref, *frames[b], None, 80, topk)
        assert ids[0] == b and sc[0] == int(frames[b][1].sum()) and cm[0] == int(bn[b]), (b, ids, sc, cm)
    db.close(), vocab.close()


@pytest.mark.gpu
def test_gpu_shifted_frames_against_the_unshifted_database(gpu_ctx):
    """The frames of test_gpu_bow_shifted_frame_end_to_end: the database holds the unshifted ones, the queries are the
    shifted ones.  Bit for bit against the reference; the rank of the origin frame is printed (nobody has measured it)."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import BowDatabase, OrbFrontend
    B, dx, dy = 4, 4, 2
    levels = synth.level_table()
    pyr = synth.make_batch(90, B)
    shifted = pyr.copy()
    for w, h, r0 in [(int(t[0]), int(t[1]), int(t[2])) for t in levels]:
        shifted[:, r0:r0 + h, :w] = np.roll(pyr[:, r0:r0 + h, :w], (dy, dx), axis=(1, 2))
    fe = OrbFrontend(levels, vstep=640, rows=2210, max_keypoints=STRIDE, ctx=gpu_ctx)
    vocab, tree = make_vocab(gpu_ctx, "b3", 8, 2)
    nwords = tree["nwords"]
    idf = np.random.default_rng(19).integers(1, 60000, nwords).astype(np.uint32)
    sides = []
    for p in (pyr, shifted):
        kp, desc, counts = fe.alloc_outputs(B, dev())
        fe(torch.from_numpy(p).to(dev()), kp, desc, counts)
        torch.cuda.synchronize()
        bw, _, bn, wt = bow_chain(gpu_ctx, vocab, host(desc), host(counts), idf, nwords)
        sides.append((bw, wt, bn))
    kf, qf = as_frames(*sides[0]), as_frames(*sides[1])
    db, ref = BowDatabase(nwords, STRIDE, B, ctx=gpu_ctx), RefDb(nwords, STRIDE, B)
    assert db.add(*[T(a) for a in sides[0]]) == ref.add(kf) == 0
    for pct in (0, 80):
        got = gpu_query(db, qf, STRIDE, B, pct)
        check_query(got, ref, qf, STRIDE, B, pct, what=("shifted", pct))
        rank = [got[0][b].view(np.int32).tolist().index(b) if b in got[0][b].view(np.int32).tolist() else -1 for b in range(B)]
        print(f"min_common_pct {pct}: rank of the origin frame per shifted query {rank}, scores {got[1][:, 0].tolist()}")
    db.close(), vocab.close()


# ---- GPU: refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_bowdb_rejects_bad_arguments(gpu_ctx):
    import ctypes
    import torch
    from pislam_amd.capi import ptr
    from pislam_amd.frontend import BowDatabase
    lib, h = gpu_ctx.lib, gpu_ctx.h
    B, S, K, nwords = 3, 16, 4, 100
    db = BowDatabase(nwords, S, 8, ctx=gpu_ctx)
    word = torch.arange(B * S, dtype=torch.int32, device=dev()).reshape(B, S) % nwords
    val = torch.full((B, S), 1000, dtype=torch.int32, device=dev())
    n = torch.full((B,), S, dtype=torch.int32, device=dev())
    lim = torch.full((B,), 8, dtype=torch.int32, device=dev())
    idf = torch.ones((nwords,), dtype=torch.int32, device=dev())
    outs = [filled((B, K)), filled((B, K)), filled((B, K)), filled((B,))]
    wout = filled((B, S))

    def untouched():
        torch.cuda.synchronize()
        return all((host(o) == SENTINEL).all() for o in outs + [wout])

    def weight(**kw):
        a = dict(word=word, tf=val, n=n, stride=S, batch=B, idf=idf, nwords=nwords, out=wout)
        a.update(kw)
        return lib.pislam_bow_weight_batch(h, ptr(a["word"]), ptr(a["tf"]), ptr(a["n"]), a["stride"], a["batch"], ptr(a["idf"]),
                                           a["nwords"], ptr(a["out"]))

    for kw in (dict(word=None), dict(tf=None), dict(n=None), dict(out=None), dict(word=word.cpu()), dict(tf=val.cpu()),
               dict(n=n.cpu()), dict(idf=idf.cpu()), dict(out=wout.cpu()), dict(batch=-1), dict(stride=16385)):
        assert weight(**kw) == -1, kw
        assert untouched()

    def query(**kw):
        a = dict(db=db.h, word=word, val=val, n=n, stride=S, batch=B, lim=lim, pct=80, topk=K, o=outs)
        a.update(kw)
        return lib.pislam_bowdb_query_batch(h, a["db"], ptr(a["word"]), ptr(a["val"]), ptr(a["n"]), a["stride"], a["batch"],
                                            ptr(a["lim"]), a["pct"], a["topk"], *[ptr(o) for o in a["o"]])

    assert db.add(word, val, n) == 0
    cases = [dict(db=None), dict(word=None), dict(val=None), dict(n=None), dict(word=word.cpu()), dict(val=val.cpu()),
             dict(n=n.cpu()), dict(lim=lim.cpu()), dict(topk=0), dict(topk=65), dict(pct=-1), dict(pct=101), dict(batch=-1),
             dict(batch=65536), dict(stride=16385)]
    for k in range(4):
        cases.append(dict(o=[None if j == k else o for j, o in enumerate(outs)]))
        cases.append(dict(o=[o.cpu() if j == k else o for j, o in enumerate(outs)]))
    for kw in cases:
        assert query(**kw) == -1, kw
        assert untouched()
    assert lib.pislam_bowdb_query_reserve(h, None, B, K) == -1 and lib.pislam_bowdb_query_reserve(h, db.h, B, 0) == -1
    assert lib.pislam_bowdb_query_reserve(h, db.h, B, 65) == -1 and lib.pislam_bowdb_query_reserve(h, db.h, -1, K) == -1
    # add: NULL / host tensors, a batch that passes the capacity; create: ranges; size / destroy of NULL
    first = ctypes.c_int32(77)
    add = lambda w=word, v=val, c=n, batch=B: lib.pislam_bowdb_add_batch(h, db.h, ptr(w), ptr(v), ptr(c), S, batch, ctypes.byref(first))
    for kw in (dict(w=None), dict(v=None), dict(c=None), dict(w=word.cpu()), dict(v=val.cpu()), dict(c=n.cpu()), dict(batch=6),
               dict(batch=-1)):
        assert add(**kw) == -1, kw
        assert db.size == B and first.value == 77
    assert lib.pislam_bowdb_add_batch(h, None, ptr(word), ptr(val), ptr(n), S, B, None) == -1
    out = ctypes.c_void_p()
    for nw, st, cap in [(0, S, 8), ((1 << 24) + 1, S, 8), (nwords, 0, 8), (nwords, 16385, 8), (nwords, S, 0), (nwords, S, (1 << 20) + 1)]:
        assert lib.pislam_bowdb_create(h, nw, st, cap, ctypes.byref(out)) == -1 and not out.value
    assert lib.pislam_bowdb_create(h, nwords, S, 8, None) == -1
    assert lib.pislam_bowdb_size(None) == -1 and lib.pislam_bowdb_destroy(None) == -1
    assert lib.pislam_bowdb_remove(h, db.h, None, 1) == -1 and lib.pislam_bowdb_clear(h, None) == -1
    assert untouched()
    assert query() == 0                                             # the baseline call is accepted
    torch.cuda.synchronize()
    assert (host(outs[0])[:, 0].view(np.int32) == np.arange(B)).all() and (host(outs[3]) == S).all()
    assert weight() == 0
    torch.cuda.synchronize()
    assert (host(wout) == Q24 // S).all()
    db.close()


@pytest.mark.gpu
def test_gpu_query_reserve_reports_no_memory(gpu_ctx):
    """A workspace that cannot be had (65535 queries against 2^20 key frames: 412 GB) is PISLAM_ERR_NOMEM, not a fault,
    and the context serves a smaller query afterwards."""
    from pislam_amd.frontend import BowDatabase
    db, ref = BowDatabase(1000, 1, 1 << 20, ctx=gpu_ctx), RefDb(1000, 1, 1 << 20)
    assert gpu_ctx.lib.pislam_bowdb_query_reserve(gpu_ctx.h, db.h, 65535, 64) == -3
    frames = [frame([w], [Q24]) for w in (5, 7, 5, 9)]
    assert gpu_add(db, frames, 1) == ref.add(frames) == 0
    check_query(gpu_query(db, frames, 1, 3, 80), ref, frames, 1, 3, 80, what="after the refused reserve")
    db.close()


# ---- GPU: hipGraph ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_bowdb_query_is_hipgraph_capturable(gpu_ctx):
    """transform + vector + weight + query captured once on a side stream (one stream, no parallel branches): the replay
    equals the eager result; key frames added OUTSIDE the graph are seen by the next replay."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import BowDatabase, bowTransformBatch, bowVectorBatch, bowWeightBatch
    B, words, topk = 4, 8, 8
    fd, fn = fe_descriptors(words)
    counts = fn.astype(np.uint32)
    side = torch.cuda.Stream(dev())
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        vocab, tree = make_vocab(ctx, "b3", words, 2)
        nwords = tree["nwords"]
        idf = np.random.default_rng(20).integers(1, 60000, nwords).astype(np.uint32)
        d_idf = T(idf)
        bw, tf, bn, wt = bow_chain(ctx, vocab, fd, counts, idf, nwords)      # all nine frames, eagerly
        side.synchronize()
        frames = as_frames(bw, wt, bn)
        db, ref = BowDatabase(nwords, STRIDE, 16, ctx=ctx), RefDb(nwords, STRIDE, 16)
        assert db.add(T(bw[:5]), T(wt[:5]), T(bn[:5])) == ref.add(frames[:5]) == 0
        db.reserve_query(B, topk)
        qd, qc = T(fd[3:3 + B]), T(counts[3:3 + B])
        z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev())
        word, vw, vtf, vn, vwt = z(B, STRIDE), z(B, STRIDE), z(B, STRIDE), z(B), z(B, STRIDE)
        outs = [z(B, topk), z(B, topk), z(B, topk), z(B)]

        def step():
            bowTransformBatch(vocab, qd, qc, word, want_group=False, want_wdist=False, ctx=ctx)
            bowVectorBatch(word, qc, vw, vtf, vn, ctx=ctx)
            bowWeightBatch(vw, vtf, vn, d_idf, nwords, vwt, ctx=ctx)
            db.query(vw, vwt, vn, topk=topk, min_common_pct=80, top_id=outs[0], top_score=outs[1], top_common=outs[2],
                     max_common=outs[3])

        step()
        side.synchronize()
        eager = [o.clone() for o in outs]
        check_query([host(o) for o in outs], ref, frames[3:3 + B], STRIDE, topk, 80, what="eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step()
        for o in outs:
            o.fill_(7)
        g.replay()
        side.synchronize()
        for a, b in zip(eager, outs):
            assert torch.equal(a, b)
        assert db.add(T(bw[5:]), T(wt[5:]), T(bn[5:])) == ref.add(frames[5:]) == 5      # outside the graph
        db.remove([4]), ref.remove([4])
        for o in outs:
            o.fill_(7)
        g.replay()
        side.synchronize()
    got = [host(o) for o in outs]
    check_query(got, ref, frames[3:3 + B], STRIDE, topk, 80, what="replay on the larger database")
    assert got[0][2, 0] == 5 and got[0][3, 0] == 6                   # frames 5 and 6 find themselves only after the add
    db.close(), vocab.close()
