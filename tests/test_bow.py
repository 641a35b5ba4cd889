"""Bag-of-words quantisation, vectors and word-guided matching (pislam_vocab_*, pislam_bow_transform_batch,
pislam_bow_vector_batch, pislam_match_hamming_bow_batch).

The semantics are the library's own (include/pislam_hip.h).  This file states them independently of the library and of
its node records: `ref_tree` validates a tree and numbers its words and groups, `ref_descend` drops descriptors down it by
an argmin over dist * 256 + child, `np.unique` is the vector, and `ref_bow_match` is a masked minimum of
dist * 65536 + j over the full nq x nt Hamming matrix.  The CPU tests check that reference on hand-built trees; the GPU
tests compare the library with it bit for bit, outputs pre-filled with a sentinel."""
import functools

import numpy as np
import pytest

from test_match_scaled_window import hamming
from test_match_window import SENTINEL, clamp_count, frontend_outputs, random_descriptors

BIG = np.int64(1) << 40
NONE_U32 = np.uint32(0xFFFFFFFF)
COUNT_INVALID = 0xFFFFFFFF
POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


# ---- the reference ---------------------------------------------------------------------------------------------------
def ref_tree(words, nnodes, first_child, child_count, group_depth):
    """Validates the tree as the header lists it (ValueError otherwise) and returns parent, depth, word id and group id
    per node (-1 where a node has none), nwords and ngroups."""
    if words not in (1, 2, 4, 8):
        raise ValueError("words")
    if not 2 <= nnodes <= 1 << 24:
        raise ValueError("nnodes")
    if not 0 <= group_depth <= 16:
        raise ValueError("group_depth")
    fc, cc = np.asarray(first_child, np.int64), np.asarray(child_count, np.int64)
    if len(fc) != nnodes or len(cc) != nnodes:
        raise ValueError("shape")
    if ((cc < 0) | (cc > 32)).any():
        raise ValueError("child_count")
    if cc[0] == 0:
        raise ValueError("root is a leaf")
    n = np.arange(nnodes, dtype=np.int64)
    inner = cc > 0
    if (inner & ((fc <= n) | (fc < 1) | (fc + cc > nnodes))).any():
        raise ValueError("child range")
    par = np.repeat(n, cc)                                          # one entry per (parent, child) edge
    kid = np.repeat(fc, cc) + np.arange(len(par)) - np.repeat(np.cumsum(cc) - cc, cc)
    times = np.bincount(kid, minlength=nnodes)
    if (times > 1).any():
        raise ValueError("overlap")
    if (times[1:] == 0).any():
        raise ValueError("orphan")
    parent = np.full(nnodes, -1, np.int64)
    parent[kid] = par
    depth = np.full(nnodes, -1, np.int64)
    depth[0] = 0
    frontier, d = np.array([0]), 0
    while True:                                                     # level by level (first_child > n: no cycles)
        f, c = fc[frontier], cc[frontier]
        nxt = np.repeat(f, c) + np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
        if not len(nxt):
            break
        d += 1
        if d > 16:
            raise ValueError("depth")
        depth[nxt] = d
        frontier = nxt
    leaf = ~inner
    word = np.full(nnodes, -1, np.int64)
    word[leaf] = np.arange(int(leaf.sum()))
    gnode = (depth == group_depth) | (leaf & (depth < group_depth))
    group = np.full(nnodes, -1, np.int64)
    group[gnode] = np.arange(int(gnode.sum()))
    for dd in range(group_depth + 1, int(depth.max()) + 1):
        sel = depth == dd
        group[sel] = group[parent[sel]]
    return dict(parent=parent, depth=depth, word=word, group=group, nwords=int(leaf.sum()), ngroups=int(gnode.sum()))


def popcount_rows(x):
    """Bits set per row of uint32 [..., words]."""
    return POP8[np.ascontiguousarray(x, np.uint32).view(np.uint8)].sum(-1)


def new_trace():
    return dict(steps=0, ties=0, max_child=-1)


def ref_descend(desc, node_desc, first_child, child_count, tree, trace=None):
    """(word, group, wdist) int64 [n] of descriptors uint32 [n][words].  trace counts the descent steps, those with an
    exact tie for the smallest distance, and the largest child index chosen."""
    n = len(desc)
    fc, cc = np.asarray(first_child, np.int64), np.asarray(child_count, np.int64)
    cur, wd = np.zeros(n, np.int64), np.zeros(n, np.int64)
    while True:
        act = np.flatnonzero(cc[cur] > 0)
        if not len(act):
            break
        f, c = fc[cur[act]], cc[cur[act]]
        slot = np.arange(int(c.max()), dtype=np.int64)[None, :]
        child = f[:, None] + np.minimum(slot, c[:, None] - 1)
        d = popcount_rows(desc[act][:, None, :] ^ node_desc[child])
        valid = slot < c[:, None]
        key = np.where(valid, d * 256 + slot, BIG)
        am = key.argmin(1)
        rows = np.arange(len(act))
        if trace is not None:
            dmin = d[rows, am]
            trace["steps"] += len(act)
            trace["ties"] += int((((d == dmin[:, None]) & valid).sum(1) > 1).sum())
            trace["max_child"] = max(trace["max_child"], int(am.max()))
        cur[act] = f + am
        wd[act] = d[rows, am]
    return tree["word"][cur], tree["group"][cur], wd


def ref_bow_match(qd, qg, td, tg, ngroups):
    """(idx int32, dist uint32, dist2 uint32) [nq] of one pair."""
    nq, nt = len(qd), len(td)
    idx = np.full(nq, -1, np.int32)
    dist = np.full(nq, NONE_U32, np.uint32)
    dist2 = np.full(nq, NONE_U32, np.uint32)
    if nq == 0 or nt == 0:
        return idx, dist, dist2
    qg, tg = np.asarray(qg, np.int64), np.asarray(tg, np.int64)
    jj = np.arange(nt, dtype=np.int64)
    step = max(1, (1 << 22) // nt)                                  # query rows per chunk: bounded memory at nt = 65535
    for a in range(0, nq, step):
        s = slice(a, min(nq, a + step))
        d = hamming(qd[s], td)
        mask = (qg[s][:, None] == tg[None, :]) & (qg[s][:, None] < ngroups) & (tg[None, :] < ngroups)
        key = np.where(mask, d * 65536 + jj[None, :], BIG)
        rows = np.arange(key.shape[0])
        am = key.argmin(1)
        best = key[rows, am].copy()
        key[rows, am] = BIG
        second = key.min(1)
        has, has2 = best < BIG, second < BIG
        idx[s] = np.where(has, best % 65536, -1).astype(np.int32)
        dist[s] = np.where(has, best // 65536, 0xFFFFFFFF).astype(np.uint32)
        dist2[s] = np.where(has2, second // 65536, 0xFFFFFFFF).astype(np.uint32)
    return idx, dist, dist2


# ---- test vocabularies (seeded, built here) ------------------------------------------------------------------------
def kary(k, depth):
    """(first_child, child_count) of the complete k-ary tree in breadth-first order, leaves at `depth`."""
    nn = sum(k ** d for d in range(depth + 1))
    inner = sum(k ** d for d in range(depth))
    n = np.arange(nn, dtype=np.int64)
    return np.where(n < inner, n * k + 1, 0).astype(np.int32), np.where(n < inner, k, 0).astype(np.int32)


def random_tree(rng, words, max_nodes=6000, max_depth=7):
    """(a): random child counts 0..32, ragged leaf depths, random node descriptors."""
    fc, cc, depth = [0], [0], [0]
    n = 0
    while n < len(fc):
        d = depth[n]
        c = int(rng.integers(1, 33)) if n == 0 else int(rng.integers(0, 33))
        if d >= max_depth or len(fc) + c > max_nodes or (n and rng.random() < 0.25):
            c = 0 if n else c
        if c:
            fc[n], cc[n] = len(fc), c
            fc += [0] * c
            cc += [0] * c
            depth += [d + 1] * c
        n += 1
    nn = len(fc)
    desc = rng.integers(0, 2**32, (nn, words), dtype=np.uint64).astype(np.uint32)
    return desc, np.array(fc, np.int32), np.array(cc, np.int32)


def kmajority_tree(rng, desc, k, depth):
    """(b): complete k-ary tree grown by hierarchical k-majority over `desc` uint32 [n][words] (three rounds per node:
    nearest centre, ties to the lowest; bitwise majority; an empty cluster keeps a random centre)."""
    words = desc.shape[1]
    fc, cc = kary(k, depth)
    nn = len(fc)
    node_desc = rng.integers(0, 2**32, (nn, words), dtype=np.uint64).astype(np.uint32)
    bits = np.unpackbits(np.ascontiguousarray(desc).view(np.uint8), axis=1)
    members = {0: np.arange(len(desc))}
    for n in range(nn):
        if cc[n] == 0:
            continue
        S = members.pop(n, np.zeros(0, np.int64))
        kids = int(fc[n]) + np.arange(k)
        if len(S) == 0:
            continue
        centres = desc[rng.choice(S, k, replace=len(S) < k)].copy()
        for _ in range(3):
            a = hamming(desc[S], centres).argmin(1)
            for c in range(k):
                m = S[a == c]
                if len(m):
                    maj = (bits[m].sum(0) * 2 > len(m)).astype(np.uint8)
                    centres[c] = np.packbits(maj).view(np.uint32)
        a = hamming(desc[S], centres).argmin(1)
        node_desc[kids] = centres
        for c in range(k):
            members[int(kids[c])] = S[a == c]
    return node_desc, fc, cc


FE_PYRAMIDS = 9


@functools.lru_cache(maxsize=None)
def fe_outputs():
    """Front-end outputs of FE_PYRAMIDS synthetic pyramids (words 8): levels, keypoints, descriptors, counts."""
    return frontend_outputs(FE_PYRAMIDS, seed=40)


def fe_descriptors(words):
    """The descriptors of fe_outputs cut to `words` dwords, [pyramids][2048][words], and their clamped counts."""
    _, _, desc, counts = fe_outputs()
    n = np.array([clamp_count(c, desc.shape[1]) for c in counts])
    return np.ascontiguousarray(desc[:, :, :words]), n


@functools.lru_cache(maxsize=None)
def host_vocab(kind, words):
    """(node_desc, first_child, child_count) of vocabulary "a", "b3", "b4" or "c"."""
    rng = np.random.default_rng([ord(kind[0]), int(kind[1:] or 0), words])
    if kind == "a":
        return random_tree(rng, words)
    if kind in ("b3", "b4"):
        desc, n = fe_descriptors(words)
        pool = np.concatenate([desc[b, :n[b]] for b in range(len(n))])
        return kmajority_tree(rng, pool, 10, int(kind[1]))
    assert kind == "c"                                              # 10-ary, depth 6: 1 111 111 nodes, 36 MB at words 8
    fc, cc = kary(10, 6)
    return rng.integers(0, 2**32, (len(fc), words), dtype=np.uint64).astype(np.uint32), fc, cc


def dev():
    import torch
    return torch.device("cuda:0")


def T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev())


def filled(shape, fill=SENTINEL):
    import torch
    return torch.full(shape, fill - (1 << 32) if fill >= 1 << 31 else fill, dtype=torch.int32, device=dev())


def host(t):
    return t.cpu().numpy().view(np.uint32)


def make_vocab(ctx, kind, words, group_depth):
    from pislam_amd.frontend import Vocabulary
    nd, fc, cc = host_vocab(kind, words)
    tree = ref_tree(words, len(fc), fc, cc, group_depth)
    v = Vocabulary(nd, fc, cc, group_depth, ctx=ctx)
    assert (v.nwords, v.ngroups) == (tree["nwords"], tree["ngroups"])
    return v, tree


# ---- CPU: the reference itself, and the Python-side checks -----------------------------------------------------------
def bits(n):
    return np.uint32((1 << n) - 1)


def test_reference_two_level_tree():
    """Root -> 3 children, the middle one has 2 children: 4 leaves (nodes 1, 3, 4, 5), words in node order."""
    fc = np.array([1, 0, 4, 0, 0, 0], np.int32)
    cc = np.array([3, 0, 2, 0, 0, 0], np.int32)
    nd = np.array([[0xDEAD], [bits(0)], [bits(16)], [bits(32)], [bits(12)], [bits(20)]], np.uint32)
    tree = ref_tree(1, 6, fc, cc, 1)
    assert tree["nwords"] == 4 and tree["ngroups"] == 3
    assert tree["word"].tolist() == [-1, 0, -1, 1, 2, 3] and tree["depth"].tolist() == [0, 1, 1, 1, 2, 2]
    assert tree["group"].tolist() == [-1, 0, 1, 2, 1, 1]
    q = np.array([[bits(1)], [bits(31)], [bits(13)], [bits(19)]], np.uint32)
    w, g, d = ref_descend(q, nd, fc, cc, tree)
    assert w.tolist() == [0, 1, 2, 3] and g.tolist() == [0, 2, 1, 1] and d.tolist() == [1, 1, 1, 1]


def test_reference_tie_goes_to_the_lower_child():
    fc, cc = np.array([1, 0, 0, 0], np.int32), np.array([3, 0, 0, 0], np.int32)
    nd = np.array([[0], [bits(8)], [bits(4)], [bits(4) << 4]], np.uint32)      # distances 8, 4, 4 to the zero descriptor
    tree = ref_tree(1, 4, fc, cc, 0)
    tr = new_trace()
    w, g, d = ref_descend(np.zeros((1, 1), np.uint32), nd, fc, cc, tree, tr)
    assert (w[0], g[0], d[0]) == (1, 0, 4) and tr == dict(steps=1, ties=1, max_child=1)
    # the root's own descriptor never takes part
    nd[0] = 0xFFFFFFFF
    assert ref_descend(np.zeros((1, 1), np.uint32), nd, fc, cc, tree)[0][0] == 1


def test_reference_group_numbering():
    """A leaf shallower than group_depth is its own group; group_depth 0 is one group; a group_depth below every leaf
    makes groups equal words."""
    #            0  1  2  3  4  5  6  7        root -> 1, 2, 3;  2 -> 4, 5;  5 -> 6, 7
    fc = np.array([1, 0, 4, 0, 0, 6, 0, 0], np.int32)
    cc = np.array([3, 0, 2, 0, 0, 2, 0, 0], np.int32)
    t2 = ref_tree(2, 8, fc, cc, 2)                                  # groups: leaves 1, 3 (depth 1), nodes 4, 5 (depth 2)
    assert t2["ngroups"] == 4 and t2["group"].tolist() == [-1, 0, -1, 1, 2, 3, 3, 3]
    assert t2["word"].tolist() == [-1, 0, -1, 1, 2, -1, 3, 4] and t2["nwords"] == 5
    t0 = ref_tree(2, 8, fc, cc, 0)
    assert t0["ngroups"] == 1 and t0["group"].tolist() == [0] * 8
    for gd in (3, 9, 16):
        t = ref_tree(2, 8, fc, cc, gd)
        leaf = cc == 0
        assert t["ngroups"] == t["nwords"] and (t["group"][leaf] == t["word"][leaf]).all()
    # ORB-SLAM's levelsup on a complete tree: 10-ary depth 3, group_depth 2 = 100 groups of 10 words
    f10, c10 = kary(10, 3)
    t = ref_tree(8, len(f10), f10, c10, 2)
    assert (t["nwords"], t["ngroups"]) == (1000, 100)
    assert (t["group"][c10 == 0] == np.arange(1000) // 10).all()


def malformed_trees():
    """(name, words, first_child, child_count, group_depth) of every refusal the header lists."""
    ok_f, ok_c = [1, 3, 0, 0, 0], [2, 2, 0, 0, 0]                   # root -> 1, 2;  1 -> 3, 4
    chain_f = list(range(1, 18)) + [0]                              # a chain of 18 nodes: the leaf is at depth 17
    chain_c = [1] * 17 + [0]
    return [
        ("words 3", 3, ok_f, ok_c, 1),
        ("one node", 8, [0], [0], 0),
        ("child_count 33", 8, [1] + [0] * 33, [33] + [0] * 33, 1),
        ("child_count -1", 8, ok_f, [2, 2, -1, 0, 0], 1),
        ("root a leaf", 8, [0, 0], [0, 0], 0),
        ("range past nnodes", 8, [1, 3, 0, 0, 0], [2, 3, 0, 0, 0], 1),
        ("range holds the root", 8, [1, 0, 0], [1, 2, 0], 1),
        ("range before the parent", 8, [2, 0, 1], [1, 0, 1], 1),
        ("child of itself", 8, [1, 1, 0], [2, 1, 0], 1),
        ("overlapping ranges", 8, [1, 3, 4, 0, 0, 0], [2, 2, 2, 0, 0, 0], 1),
        ("orphan", 8, [1, 0, 0, 0], [2, 0, 0, 0], 1),
        ("depth 17", 8, chain_f, chain_c, 1),
        ("group_depth 17", 8, ok_f, ok_c, 17),
        ("group_depth -1", 8, ok_f, ok_c, -1),
    ]


def test_reference_refuses_malformed_trees():
    ref_tree(8, 5, [1, 3, 0, 0, 0], [2, 2, 0, 0, 0], 1)
    ref_tree(8, 17, list(range(1, 17)) + [0], [1] * 16 + [0], 16)   # depth 16 is allowed
    for name, words, fc, cc, gd in malformed_trees():
        with pytest.raises(ValueError):
            print(name)
            ref_tree(words, len(fc), fc, cc, gd)
    for seed in range(5):
        nd, fc, cc = random_tree(np.random.default_rng(seed), 2, max_nodes=500)
        t = ref_tree(2, len(fc), fc, cc, 3)
        assert t["nwords"] == int((cc == 0).sum()) and 1 <= t["depth"].max() <= 7


def test_reference_matcher_hand_built_cases():
    td = np.array([[bits(4)], [bits(1)], [bits(9)], [bits(1)], [bits(0)]], np.uint32)
    tg = [0, 1, 1, 1, 7]
    q = np.zeros((3, 1), np.uint32)
    i, d, d2 = ref_bow_match(q, [1, 0, 7], td, tg, 5)
    assert (i[0], d[0], d2[0]) == (1, 1, 1)                         # a duplicate: the smallest index, dist2 its twin
    assert (i[1], d[1], d2[1]) == (0, 4, NONE_U32)                  # one candidate
    assert (i[2], d[2], d2[2]) == (-1, NONE_U32, NONE_U32)          # id 7 >= ngroups on both sides: no candidates
    i, d, d2 = ref_bow_match(q, [0, 0, 0], td, [0] * 5, 1)          # one group: brute force
    assert (i == 4).all() and (d == 0).all() and (d2 == 1).all()


def test_python_side_shape_checks_need_no_device():
    """Vocabulary checks the array shapes before it touches the library."""
    from pislam_amd.frontend import Vocabulary
    good = np.zeros((5, 8), np.uint32)
    for nd, fc, cc in [(np.zeros(5, np.uint32), [1, 3, 0, 0, 0], [2, 2, 0, 0, 0]),          # not [nnodes][words]
                       (np.zeros((5, 3), np.uint32), [1, 3, 0, 0, 0], [2, 2, 0, 0, 0]),     # words 3
                       (good, [1, 3, 0, 0], [2, 2, 0, 0, 0]),                               # first_child too short
                       (good, [1, 3, 0, 0, 0], [2, 2, 0, 0, 0, 0])]:                        # child_count too long
        with pytest.raises(ValueError):
            Vocabulary(nd, fc, cc, 1)
    with pytest.raises(ValueError):
        Vocabulary.from_kary(np.zeros((110, 8), np.uint32), 10, 2)  # a 10-ary tree of depth 2 has 111 nodes
    for k, depth in [(10, 3), (2, 5), (32, 2), (1, 4)]:
        f, c = Vocabulary.kary_tables(k, depth)
        ef, ec = kary(k, depth)
        assert (f == ef).all() and (c == ec).all()
        ref_tree(8, len(f), f, c, 1)


# ---- GPU: vocabulary ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_vocab_create_refuses_malformed_trees(gpu_ctx):
    import ctypes
    from pislam_amd.capi import PislamError
    from pislam_amd.frontend import Vocabulary
    lib = gpu_ctx.lib
    for name, words, fc, cc, gd in malformed_trees():
        nd = np.zeros((len(fc), words), np.uint32)
        f, c = np.array(fc, np.int32), np.array(cc, np.int32)
        h = ctypes.c_void_p()
        rc = lib.pislam_vocab_create(gpu_ctx.h, words, len(fc), nd.ctypes.data, f.ctypes.data, c.ctypes.data, gd, ctypes.byref(h))
        assert rc == -1 and not h.value, name
    nd = np.zeros((5, 8), np.uint32)
    f, c = np.array([1, 3, 0, 0, 0], np.int32), np.array([2, 2, 0, 0, 0], np.int32)
    h = ctypes.c_void_p()
    assert lib.pislam_vocab_create(gpu_ctx.h, 8, 5, None, f.ctypes.data, c.ctypes.data, 1, ctypes.byref(h)) == -1
    assert lib.pislam_vocab_create(gpu_ctx.h, 8, 5, nd.ctypes.data, f.ctypes.data, c.ctypes.data, 1, None) == -1
    assert lib.pislam_vocab_create(gpu_ctx.h, 8, 1 << 24 | 1, nd.ctypes.data, f.ctypes.data, c.ctypes.data, 1, ctypes.byref(h)) == -1
    assert lib.pislam_vocab_nwords(None) == -1 and lib.pislam_vocab_ngroups(None) == -1 and lib.pislam_vocab_destroy(None) == -1
    with pytest.raises(PislamError):
        Vocabulary(nd, [1, 3, 0, 0, 0], [2, 2, 0, 0, 1], 1, ctx=gpu_ctx)
    # accepted: the deepest tree, every group_depth, and the counts agree with the reference
    chain_f, chain_c = list(range(1, 17)) + [0], [1] * 16 + [0]
    for gd in (0, 5, 16):
        v = Vocabulary(np.zeros((17, 1), np.uint32), chain_f, chain_c, gd, ctx=gpu_ctx)
        assert (v.nwords, v.ngroups) == (1, 1)
        v.close()
    for seed in range(3):
        nd, fc, cc = random_tree(np.random.default_rng(seed), 2, max_nodes=800)
        for gd in (0, 2, 4, 16):
            t = ref_tree(2, len(fc), fc, cc, gd)
            v = Vocabulary(nd, fc, cc, gd, ctx=gpu_ctx)
            assert (v.nwords, v.ngroups) == (t["nwords"], t["ngroups"])
            v.close()


# ---- GPU: transform ----------------------------------------------------------------------------------------------------
STRIDE = 2048


def transform_inputs(words, seed):
    """Six pyramids at stride 2048: four of the front end's (one count 0, one PISLAM_COUNT_INVALID) and two of random
    descriptors (one count above the stride)."""
    rng = np.random.default_rng([words, seed])
    fd, fn = fe_descriptors(words)
    desc = np.zeros((6, STRIDE, words), np.uint32)
    desc[:4] = fd[:4]
    desc[4] = random_descriptors(rng, STRIDE, words)
    desc[5] = rng.integers(0, 2**32, (STRIDE, words), dtype=np.uint64).astype(np.uint32)
    counts = np.array([fn[0], fn[1], 0, COUNT_INVALID, 3000, 777], np.uint32)
    return desc, counts


def run_transform(ctx, vocab, desc, counts, want_group=True, want_wdist=True):
    import torch
    from pislam_amd.frontend import bowTransformBatch
    B, S, _ = desc.shape
    w, g, d = filled((B, S)), filled((B, S)) if want_group else None, filled((B, S)) if want_wdist else None
    bowTransformBatch(vocab, T(desc), T(counts), w, g, d, want_group=want_group, want_wdist=want_wdist, ctx=ctx)
    torch.cuda.synchronize()
    return [None if t is None else host(t) for t in (w, g, d)]


def check_transform(got, desc, counts, host_v, tree, trace=None):
    nd, fc, cc = host_v
    for b in range(desc.shape[0]):
        n = clamp_count(counts[b], desc.shape[1])
        exp = ref_descend(desc[b, :n], nd, fc, cc, tree, trace)
        for name, g, e in zip(("word", "group", "wdist"), got, exp):
            if g is None:
                continue
            print(f"pyramid {b}: {name} mismatches {int((g[b, :n] != e).sum())} of {n}")
            assert (g[b, :n] == e).all(), (name, b, np.flatnonzero(g[b, :n] != e)[:5])
            assert (g[b, n:] == SENTINEL).all(), ("slot past the count written", name, b)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["a", "b3", "b4", "c"])
@pytest.mark.parametrize("words", [1, 2, 4, 8])
def test_gpu_transform_matches_reference(gpu_ctx, kind, words):
    group_depth = {"a": 3, "b3": 2, "b4": 3, "c": 2}[kind]
    vocab, tree = make_vocab(gpu_ctx, kind, words, group_depth)
    desc, counts = transform_inputs(words, 1)
    trace = new_trace()
    got = run_transform(gpu_ctx, vocab, desc, counts)
    check_transform(got, desc, counts, host_vocab(kind, words), tree, trace)
    print(f"trace {kind} words {words}: {trace}")
    assert trace["steps"] >= 5000
    if words <= 2:
        assert trace["ties"] >= 1, "no descent step with an exact tie: the tie rule is not tested"
    if kind == "a":
        assert trace["max_child"] >= 16, "no chosen child with index >= 16: the second child of a lane is not tested"
    # group / wdist NULL: the other outputs do not change
    w_only = run_transform(gpu_ctx, vocab, desc, counts, want_group=False, want_wdist=False)
    assert (w_only[0] == got[0]).all() and w_only[1] is None and w_only[2] is None
    no_d = run_transform(gpu_ctx, vocab, desc, counts, want_wdist=False)
    assert (no_d[0] == got[0]).all() and (no_d[1] == got[1]).all()
    vocab.close()


@pytest.mark.gpu
def test_gpu_transform_every_group_depth(gpu_ctx):
    """One ragged tree, group_depth 0 .. 8 and 16: the group output follows the reference's numbering."""
    desc, counts = transform_inputs(2, 2)
    for gd in (0, 1, 2, 4, 7, 8, 16):
        vocab, tree = make_vocab(gpu_ctx, "a", 2, gd)
        got = run_transform(gpu_ctx, vocab, desc, counts)
        check_transform(got, desc, counts, host_vocab("a", 2), tree)
        vocab.close()


# ---- GPU: vector -------------------------------------------------------------------------------------------------------
def run_vector(ctx, word, counts):
    import torch
    from pislam_amd.frontend import bowVectorBatch
    B, S = word.shape
    bw, tf, bn = filled((B, S)), filled((B, S)), filled((B,))
    bowVectorBatch(T(word), T(counts), bw, tf, bn, ctx=ctx)
    torch.cuda.synchronize()
    return host(bw), host(tf), host(bn)


def check_vector(got, word, counts):
    bw, tf, bn = got
    for b in range(word.shape[0]):
        n = clamp_count(counts[b], word.shape[1])
        u, c = np.unique(word[b, :n], return_counts=True)
        assert bn[b] == len(u), (b, bn[b], len(u))
        assert (bw[b, :len(u)] == u).all() and (tf[b, :len(u)] == c).all(), b
        assert (bw[b, len(u):] == SENTINEL).all() and (tf[b, len(u):] == SENTINEL).all(), ("slot past bow_n written", b)


@pytest.mark.gpu
def test_gpu_vector_on_transform_output(gpu_ctx):
    for kind, words in (("b3", 8), ("a", 1), ("b4", 4)):
        vocab, tree = make_vocab(gpu_ctx, kind, words, 2)
        desc, counts = transform_inputs(words, 3)
        word = run_transform(gpu_ctx, vocab, desc, counts)[0]
        check_vector(run_vector(gpu_ctx, word, counts), word, counts)
        vocab.close()


@pytest.mark.gpu
def test_gpu_vector_hand_made_words(gpu_ctx):
    from pislam_amd.capi import PislamError
    rng = np.random.default_rng(16384)
    for S in (16384, 1000, 1):
        word = np.zeros((7, S), np.uint32)
        word[0] = 12345                                                          # all equal
        word[1] = rng.permutation(S).astype(np.uint32) * 3 + 1                   # all distinct
        word[2] = rng.integers(0, 50, S)                                         # long runs
        word[3] = rng.choice(np.array([0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000], np.uint32), S)   # the padding's value is a word too
        word[4] = rng.integers(0, 2**32, S, dtype=np.uint64).astype(np.uint32)
        word[5] = rng.integers(0, 1000000, S)
        word[6] = rng.integers(0, 10, S)
        counts = np.array([S, S, S, S + 5, S // 2 + 1, 0, COUNT_INVALID], np.uint32)
        check_vector(run_vector(gpu_ctx, word, counts), word, counts)
        counts = np.array([min(S, 3), min(S, 65), S, max(S - 1, 0), 1, 1, 2], np.uint32)
        check_vector(run_vector(gpu_ctx, word, counts), word, counts)
    word = np.zeros((1, 16385), np.uint32)
    with pytest.raises(PislamError):
        run_vector(gpu_ctx, word, np.array([10], np.uint32))


@pytest.mark.gpu
def test_gpu_vector_scan_at_chunk_sizes(gpu_ctx):
    """The run-head scan with one word, with chunks of 2 of which most are empty (1025 words, all distinct and all
    equal) and with full chunks of 16 (16384 distinct words)."""
    rng = np.random.default_rng(1025)
    S = 16384
    word = np.zeros((4, S), np.uint32)
    word[0] = 7
    word[1] = rng.permutation(S).astype(np.uint32) * 5 + 2
    word[2] = 99
    word[3] = rng.permutation(S).astype(np.uint32) * 3
    counts = np.array([1, 1025, 1025, S], np.uint32)
    got = run_vector(gpu_ctx, word, counts)
    check_vector(got, word, counts)
    assert list(got[2]) == [1, 1025, 1, S]


# ---- GPU: word-guided matcher ------------------------------------------------------------------------------------------
def run_bow_match(ctx, ngroups, qd, qg, qc, td, tg, tc, fill=SENTINEL):
    import torch
    from pislam_amd.frontend import matchHammingBowBatch
    B, qs = qg.shape
    outs = [filled((B, qs), fill) for _ in range(3)]
    matchHammingBowBatch(T(qd), T(qg), T(qc), T(td), T(tg), T(tc), ngroups, *outs, ctx=ctx)
    torch.cuda.synchronize()
    return [host(o) for o in outs]


def check_bow_match(got, ngroups, qd, qg, qc, td, tg, tc, fill=SENTINEL):
    gi, gd, g2 = got
    qs, ts = qg.shape[1], tg.shape[1]
    for b in range(qg.shape[0]):
        nq, nt = clamp_count(qc[b], qs), clamp_count(tc[b], ts)
        ei, ed, e2 = ref_bow_match(qd[b, :nq], qg[b, :nq], td[b, :nt], tg[b, :nt], ngroups)
        assert (gi[b, :nq].view(np.int32) == ei).all(), (b, ngroups, np.flatnonzero(gi[b, :nq].view(np.int32) != ei)[:5])
        assert (gd[b, :nq] == ed).all(), (b, ngroups)
        assert (g2[b, :nq] == e2).all(), (b, ngroups)
        for g in (gi, gd, g2):
            assert (g[b, nq:] == fill).all(), ("slot past the query count written", b)


@pytest.mark.gpu
@pytest.mark.parametrize("words", [1, 2, 4, 8])
def test_gpu_bow_match_one_group_is_brute_force(gpu_ctx, words):
    import torch
    from pislam_amd.frontend import matchHammingBatch
    rng = np.random.default_rng([1, words])
    pairs = [(0, 5), (5, 0), (1, 1), (63, 64), (65, 63), (1000, 1000), (1000, 1), (1, 1000)]
    B, S = len(pairs), 1000
    qd = np.stack([random_descriptors(rng, S, words) for _ in range(B)])
    td = np.stack([random_descriptors(rng, S, words) for _ in range(B)])
    qc = np.array([p[0] for p in pairs], np.uint32)
    tc = np.array([p[1] for p in pairs], np.uint32)
    zero = np.zeros((B, S), np.uint32)
    got = run_bow_match(gpu_ctx, 1, qd, zero, qc, td, zero, tc)
    check_bow_match(got, 1, qd, zero, qc, td, zero, tc)
    bf = [filled((B, S)) for _ in range(3)]
    matchHammingBatch(T(qd), T(qc), T(td), T(tc), *bf, ctx=gpu_ctx)
    torch.cuda.synchronize()
    for a, b in zip(got, bf):
        assert (a == host(b)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,group_depth,ngroups", [("b3", 2, 100), ("b3", 3, 1000), ("b4", 3, 16384)])
def test_gpu_bow_match_on_frontend_outputs(gpu_ctx, kind, group_depth, ngroups):
    """Frame k against frame k + 1 of the front end's own outputs, groups from the transform: ragged counts, one empty
    train side, one query count above the stride."""
    words, B = 8, 8
    vocab, tree = make_vocab(gpu_ctx, kind, words, group_depth)
    assert vocab.ngroups <= ngroups
    fd, fn = fe_descriptors(words)
    counts = fn.astype(np.uint32)
    group = run_transform(gpu_ctx, vocab, fd, counts)[1]
    nd, fc, cc = host_vocab(kind, words)
    for b in (0, B):
        assert (group[b, :fn[b]] == ref_descend(fd[b, :fn[b]], nd, fc, cc, tree)[1]).all()
    qd, qg, qc = fd[:B].copy(), group[:B].copy(), counts[:B].copy()
    td, tg, tc = fd[1:].copy(), group[1:].copy(), counts[1:].copy()
    # the condition on the inputs, on the reference's own candidate counts (before the count edge cases below)
    two, none, total = 0, 0, 0
    for b in range(B):
        cand = (qg[b, :qc[b], None] == tg[b, None, :tc[b]]).sum(1)
        two, none, total = two + int((cand >= 2).sum()), none + int((cand == 0).sum()), total + len(cand)
    print(f"{kind} group_depth {group_depth}: {total} queries, {two} with >= 2 candidates, {none} with none")
    assert 4 * two >= total, "fewer than a quarter of the queries have two candidates: dist2 is hardly tested"
    assert none >= 1, "every query has a candidate: the sentinels are not tested"
    tc[2] = 0
    qc[3] = 3000
    qg[4, 5:9] = SENTINEL                                           # slots a transform never wrote (ids >= ngroups)
    got = run_bow_match(gpu_ctx, ngroups, qd, qg, qc, td, tg, tc)
    check_bow_match(got, ngroups, qd, qg, qc, td, tg, tc)
    vocab.close()


@pytest.mark.gpu
@pytest.mark.parametrize("words", [1, 2, 4, 8])
@pytest.mark.parametrize("ngroups", [100, 1000, 16384])
def test_gpu_bow_match_random_groups(gpu_ctx, words, ngroups):
    """Random group ids, some at and above ngroups on either side, some groups crowded."""
    rng = np.random.default_rng([2, words, ngroups])
    pairs = [(0, 5), (5, 0), (1, 1), (63, 64), (64, 65), (1500, 1500), (1500, 1), (1, 1500), (700, 1300), (64, COUNT_INVALID)]
    B, S = len(pairs), 1500
    qd = np.stack([random_descriptors(rng, S, words) for _ in range(B)])
    td = np.stack([random_descriptors(rng, S, words) for _ in range(B)])

    def groups():
        g = rng.integers(0, ngroups + 8, (B, S))
        g = np.where(rng.random((B, S)) < 0.3, rng.integers(0, 12, (B, S)) * (ngroups // 12), g)   # crowded groups
        g = np.where(rng.random((B, S)) < 0.05, rng.choice([ngroups - 1, ngroups, 0xFFFFFFFF, 0x80000000], (B, S)), g)
        return g.astype(np.uint32)

    qg, tg = groups(), groups()
    qc = np.array([p[0] for p in pairs], np.uint32)
    tc = np.array([p[1] for p in pairs], np.uint32)
    for fill in (SENTINEL, 0):
        got = run_bow_match(gpu_ctx, ngroups, qd, qg, qc, td, tg, tc, fill=fill)
        check_bow_match(got, ngroups, qd, qg, qc, td, tg, tc, fill=fill)
    assert (got[0][5, :1500].view(np.int32) >= 0).any() and (got[0][5, :1500].view(np.int32) == -1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("ngroups", [1, 1025, 16384])
def test_gpu_bow_index_sort_bin_counts(gpu_ctx, ngroups):
    """The index kernel's counting sort with a single bin, with chunks of 2 of which most are empty and at the
    histogram's limit; three pairs with different counts (so each pair's offset row is its own): no train entry under
    live queries, every train entry in the last group, and train groups of which a third are at or above ngroups."""
    rng = np.random.default_rng([3, ngroups])
    words, qs, ts = 2, 200, 300
    qc = np.array([200, 150, 180], np.uint32)
    tc = np.array([0, 257, 300], np.uint32)
    td = np.stack([random_descriptors(rng, ts, words) for _ in range(3)])
    qd = np.stack([td[b, rng.integers(0, ts, qs)] for b in range(3)])
    tg = rng.integers(0, ngroups, (3, ts)).astype(np.uint32)
    tg[1] = ngroups - 1
    above = rng.choice(np.array([ngroups, ngroups + 7, 0x80000000, 0xFFFFFFFF], np.uint32), ts)
    tg[2] = np.where(np.arange(ts) % 3 == 0, above, tg[2])
    qg = np.stack([tg[b, rng.integers(0, ts, qs)] for b in range(3)])       # (a third of pair 2's are not groups)
    qg[1, ::4] = rng.integers(0, ngroups, len(qg[1, ::4]))
    got = run_bow_match(gpu_ctx, ngroups, qd, qg, qc, td, tg, tc)
    check_bow_match(got, ngroups, qd, qg, qc, td, tg, tc)
    gi = got[0].view(np.int32)
    assert (gi[0, :200] == -1).all()
    assert (gi[1, :150] >= 0).any() and (gi[2, :180] >= 0).any() and (gi[2, :180] == -1).any()


@pytest.mark.gpu
def test_gpu_bow_match_full_train_stride(gpu_ctx):
    """t_stride = 65535 (the largest index the dist << 16 | index key holds), one pair filled to the stride."""
    rng = np.random.default_rng(65535)
    ts, qs, words, ngroups = 65535, 200, 4, 1000
    td = np.zeros((2, ts, words), np.uint32)
    tg = np.zeros((2, ts), np.uint32)
    td[0] = random_descriptors(rng, ts, words)
    tg[0] = rng.integers(0, ngroups + 3, ts)
    td[1, :100] = random_descriptors(rng, 100, words)
    tg[1, :100] = rng.integers(0, 5, 100)
    qd = np.stack([random_descriptors(rng, qs, words) for _ in range(2)])
    qg = np.stack([rng.integers(0, ngroups + 3, qs), rng.integers(0, 6, qs)]).astype(np.uint32)
    qd[0, :65], qg[0, :65] = td[0, ts - 65:], tg[0, ts - 65:]       # find the last indices
    qc, tc = np.array([qs, qs], np.uint32), np.array([ts, 100], np.uint32)
    got = run_bow_match(gpu_ctx, ngroups, qd, qg, qc, td, tg, tc)
    check_bow_match(got, ngroups, qd, qg, qc, td, tg, tc)
    got = run_bow_match(gpu_ctx, 1, qd, qg * 0, qc, td, tg * 0, tc)
    check_bow_match(got, 1, qd, qg * 0, qc, td, tg * 0, tc)


# ---- GPU: end to end, bad arguments, graphs ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_bow_shifted_frame_end_to_end(gpu_ctx):
    """Frame k against frame k with every level's content shifted by (4, 2) pixels (even: the 2 x 2 suppression blocks
    keep their alignment), both through the front end: every descriptor that is bit-identical in both frames gets the
    same word, and the guided match finds it with dist 0."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    B, dx, dy = 4, 4, 2
    levels = synth.level_table()
    pyr = synth.make_batch(90, B)
    shifted = pyr.copy()
    for w, h, r0 in [(int(t[0]), int(t[1]), int(t[2])) for t in levels]:
        shifted[:, r0:r0 + h, :w] = np.roll(pyr[:, r0:r0 + h, :w], (dy, dx), axis=(1, 2))
    fe = OrbFrontend(levels, vstep=640, rows=2210, max_keypoints=STRIDE, ctx=gpu_ctx)
    outs = []
    for p in (pyr, shifted):
        kp, desc, counts = fe.alloc_outputs(B, dev())
        fe(torch.from_numpy(p).to(dev()), kp, desc, counts)
        torch.cuda.synchronize()
        outs.append((host(desc), host(counts)))
    (qd, qc), (td, tc) = outs
    vocab, tree = make_vocab(gpu_ctx, "b3", 8, 2)
    qw, qg, _ = run_transform(gpu_ctx, vocab, qd, qc)
    tw, tg, _ = run_transform(gpu_ctx, vocab, td, tc)
    gi, gd, _ = run_bow_match(gpu_ctx, vocab.ngroups, qd, qg, qc, td, tg, tc)
    same = 0
    for b in range(B):
        nq, nt = clamp_count(qc[b], STRIDE), clamp_count(tc[b], STRIDE)
        tmap = {}
        for j in range(nt):
            tmap.setdefault(td[b, j].tobytes(), j)
        for i in range(nq):
            j = tmap.get(qd[b, i].tobytes())
            if j is None:
                continue
            same += 1
            assert qw[b, i] == tw[b, j] and qg[b, i] == tg[b, j]
            assert gd[b, i] == 0 and (td[b, gi[b, i]] == qd[b, i]).all() and gi[b, i] <= j
    print(f"bit-identical descriptors in both frames: {same}")
    assert same >= 100 * B, "the shifted frames share too few descriptors for the property to mean anything"
    vocab.close()


@pytest.mark.gpu
def test_gpu_bow_rejects_bad_arguments(gpu_ctx):
    import torch
    from pislam_amd.capi import PislamError, ptr
    from pislam_amd.frontend import (bowTransformBatch, bowVectorBatch, matchHammingBowBatch, reserveMatchBow)
    lib = gpu_ctx.lib
    B, S, words = 2, 16, 8
    vocab, _ = make_vocab(gpu_ctx, "a", words, 2)
    vocab2, _ = make_vocab(gpu_ctx, "a", 2, 2)
    desc = torch.zeros((B, S, words), dtype=torch.int32, device=dev())
    cnt = torch.full((B,), S, dtype=torch.int32, device=dev())
    grp = torch.zeros((B, S), dtype=torch.int32, device=dev())
    outs = [filled((B, S)) for _ in range(3)]
    num = filled((B,))

    def untouched():
        torch.cuda.synchronize()
        return all((host(o) == SENTINEL).all() for o in outs + [num])

    # transform
    for kw in (dict(desc=desc.cpu()), dict(counts=cnt.cpu()), dict(word=outs[0].cpu()), dict(group=outs[1].cpu()),
               dict(wdist=outs[2].cpu())):
        a = dict(desc=desc, counts=cnt, word=outs[0], group=outs[1], wdist=outs[2])
        a.update(kw)
        with pytest.raises(PislamError):
            bowTransformBatch(vocab, a["desc"], a["counts"], a["word"], a["group"], a["wdist"], ctx=gpu_ctx)
        assert untouched()
    with pytest.raises(ValueError):
        bowTransformBatch(vocab2, desc, cnt, *outs, ctx=gpu_ctx)    # a vocabulary of another `words`
    assert lib.pislam_bow_transform_batch(gpu_ctx.h, vocab.h, ptr(desc), ptr(cnt), S, B, None, ptr(outs[1]), ptr(outs[2])) == -1
    assert lib.pislam_bow_transform_batch(gpu_ctx.h, None, ptr(desc), ptr(cnt), S, B, ptr(outs[0]), None, None) == -1
    assert lib.pislam_bow_transform_batch(gpu_ctx.h, vocab.h, ptr(desc), ptr(cnt), S, -1, ptr(outs[0]), None, None) == -1
    assert untouched()
    # vector
    for kw in (dict(word=grp.cpu()), dict(counts=cnt.cpu()), dict(bw=outs[0].cpu()), dict(tf=outs[1].cpu()), dict(n=num.cpu())):
        a = dict(word=grp, counts=cnt, bw=outs[0], tf=outs[1], n=num)
        a.update(kw)
        with pytest.raises(PislamError):
            bowVectorBatch(a["word"], a["counts"], a["bw"], a["tf"], a["n"], ctx=gpu_ctx)
        assert untouched()
    assert lib.pislam_bow_vector_batch(gpu_ctx.h, ptr(grp), ptr(cnt), S, B, ptr(outs[0]), ptr(outs[1]), None) == -1
    assert lib.pislam_bow_vector_batch(gpu_ctx.h, ptr(grp), ptr(cnt), S, B, None, ptr(outs[1]), ptr(num)) == -1
    assert untouched()

    # matcher
    def call(qd=desc, qg=grp, qc=cnt, td=desc, tg=grp, tc=cnt, ngroups=100, o=outs):
        matchHammingBowBatch(qd, qg, qc, td, tg, tc, ngroups, *o, ctx=gpu_ctx)

    d3 = torch.zeros((B, S, 3), dtype=torch.int32, device=dev())
    big_d = torch.zeros((B, 65536, words), dtype=torch.int32, device=dev())
    big_g = torch.zeros((B, 65536), dtype=torch.int32, device=dev())
    for kw in (dict(ngroups=16385), dict(ngroups=0), dict(ngroups=-1), dict(qd=d3, td=d3), dict(td=big_d, tg=big_g),
               dict(qd=desc.cpu()), dict(qg=grp.cpu()), dict(qc=cnt.cpu()), dict(td=desc.cpu()), dict(tg=grp.cpu()),
               dict(tc=cnt.cpu()), dict(o=[outs[0].cpu(), outs[1], outs[2]]), dict(o=[outs[0], outs[1].cpu(), outs[2]]),
               dict(o=[outs[0], outs[1], outs[2].cpu()])):
        with pytest.raises(PislamError):
            call(**kw)
        assert untouched()
    assert lib.pislam_match_hamming_bow_batch(gpu_ctx.h, words, 100, ptr(desc), ptr(grp), ptr(cnt), S, ptr(desc), ptr(grp),
                                              ptr(cnt), S, B, ptr(outs[0]), None, ptr(outs[2])) == -1
    assert untouched()
    for kw in (dict(words=3), dict(ngroups=16385), dict(ngroups=0), dict(t_stride=65536), dict(batch=-1)):
        a = dict(ngroups=100, t_stride=S, batch=B, words=words)
        a.update(kw)
        with pytest.raises(PislamError):
            reserveMatchBow(a["ngroups"], a["t_stride"], a["batch"], words=a["words"], ctx=gpu_ctx)
    call()                                                          # the baseline call is accepted
    torch.cuda.synchronize()
    assert (host(outs[0])[:, :S].view(np.int32) == 0).all() and (host(outs[1]) == 0).all()
    vocab.close(), vocab2.close()


@pytest.mark.gpu
def test_gpu_bow_calls_are_hipgraph_capturable(gpu_ctx):
    """The transform has no workspace, the matcher none after pislam_match_bow_reserve: capture transform (query and
    train side) + match on a side stream (one stream, no parallel branches), zero the outputs, replay and compare;
    change the inputs in place, replay again and compare with the reference."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import bowTransformBatch, matchHammingBowBatch, reserveMatchBow
    B, words = 4, 8
    fd, fn = fe_descriptors(words)
    counts = fn.astype(np.uint32)
    nd, fc, cc = host_vocab("b3", words)
    qd, qc, td, tc = T(fd[:B]), T(counts[:B]), T(fd[1:B + 1]), T(counts[1:B + 1])
    side = torch.cuda.Stream(dev())
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        vocab, tree = make_vocab(ctx, "b3", words, 2)
        reserveMatchBow(vocab.ngroups, STRIDE, B, words=words, ctx=ctx)
        qo = [torch.zeros((B, STRIDE), dtype=torch.int32, device=dev()) for _ in range(3)]
        to = [torch.zeros((B, STRIDE), dtype=torch.int32, device=dev()) for _ in range(3)]
        mo = [torch.zeros((B, STRIDE), dtype=torch.int32, device=dev()) for _ in range(3)]

        def step():
            bowTransformBatch(vocab, qd, qc, *qo, ctx=ctx)
            bowTransformBatch(vocab, td, tc, *to, ctx=ctx)
            matchHammingBowBatch(qd, qo[1], qc, td, to[1], tc, vocab.ngroups, *mo, ctx=ctx)

        step()                                                      # warm-up (module load)
        side.synchronize()
        ref = [o.clone() for o in qo + to + mo]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step()
        for o in qo + to + mo:
            o.zero_()
        g.replay()
        side.synchronize()
        for a, b in zip(ref, qo + to + mo):
            assert torch.equal(a, b)
        for o in qo + to + mo:
            o.zero_()
        qd.copy_(T(fd[2:B + 2])), qc.copy_(T(counts[2:B + 2]))      # new inputs in the same buffers
        td.copy_(T(fd[3:B + 3])), tc.copy_(T(counts[3:B + 3]))
        g.replay()
        side.synchronize()
    for b in range(B):
        n = fn[2 + b]
        w, gr, d = ref_descend(fd[2 + b, :n], nd, fc, cc, tree)
        assert (host(qo[0])[b, :n] == w).all() and (host(qo[1])[b, :n] == gr).all() and (host(qo[2])[b, :n] == d).all()
        assert (host(qo[0])[b, n:] == 0).all()
    check_bow_match([host(o) for o in mo], vocab.ngroups, fd[2:B + 2], host(qo[1]), counts[2:B + 2], fd[3:B + 3],
                    host(to[1]), counts[3:B + 3], fill=0)
    vocab.close()
