"""The batched covisibility graph (pislam_covisibility_batch): weights, ordered neighbours, spanning tree, culling statistic.

ref_map below restates the contract, the comment above pislam_covisibility_batch in include/pislam_hip.h, from that comment
and not from the kernels: for every point the set of its observers (a dictionary of sets), and from that every output.  It is
integer counting, so every comparison in this file is word for word; nothing has a tolerance.

CPU: the host probe tools/probes/covis_host_check.cpp (the kernels' own rules, pislam_covis_math.h, under the host compiler)
against the restatement on the whole case list; mapObservations and essentialPairs against brute force; the wrapper's
refusals; the declarations.  GPU: the library against the restatement on the same case list (the 4096 limit case against
the probe, which the CPU test pins to the restatement), numpy inputs against tensors, a stale workspace, the grid passes of
both kernels, capture into a graph, and the chain into the pose graph.

A BATCH here is a dict of host arrays as the call takes them: pt int32 and kf uint16 [B][S], level and mask uint8 [B][S] or
None, counts and nk int32 [B], and the key-frame stride ks.  Slots behind a map's observations hold rubbish that must not be
read.  A RESULT is a dict of the seven outputs as int64 arrays, where a word of nb_idx / nb_weight that the call must not
write holds the sentinel the outputs were filled with."""
import bisect
import collections
import ctypes
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT

SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A
NO_PARENT = 0xFFFF
ORB = (15, 3, 1)                                # ORB-SLAM's min_weight, cull_min_observers, cull_level_slack
NAMES = ("nb_idx", "nb_weight", "nb_count", "parent", "kf_points", "kf_redundant", "status")
# the launch caps of pislam_amd/csrc/pislam_covis_kernels.h: CV_GRID_CAP workgroups per launch of either kernel, CV_THREADS
# threads (observation slots) per workgroup of the count kernel, one (map, key frame) per workgroup of the row kernel
CV_THREADS, CV_GRID_CAP = 256, 1024


# ---- the restatement ----------------------------------------------------------------------------------------------------
def ref_map(pt, kf, level, mask, count, nk, ks, prm, nbs):
    """One map: pt, kf (and level, mask or None) are its row of the batch, `count` and `nk` the words of counts and
    kf_counts as given."""
    min_weight, min_observers, slack = prm
    stride = len(pt)
    out = dict(status=0, nb_count=np.zeros(ks, np.int64), parent=np.full(ks, NO_PARENT, np.int64),
               kf_points=np.zeros(ks, np.int64), kf_redundant=np.zeros(ks, np.int64),
               nb_idx=np.full((ks, nbs), SENT16, np.int64), nb_weight=np.full((ks, nbs), SENT32, np.int64))
    bad = not (0 <= count <= stride and 0 <= nk <= ks)
    if not bad:
        obs = list(zip(pt[:count].tolist(), kf[:count].tolist()))
        bad = any(p < 0 or k >= nk for p, k in obs) or any(a >= b for a, b in zip(obs, obs[1:]))
    if bad:
        out["status"] = 3
        return out
    if nk == 0 or count == 0:
        out["status"] = 1
        return out
    observers, lev = {}, {}                     # point -> the set of its observers; (point, key frame) -> level
    for o, l in zip(obs, [0] * count if level is None else level[:count].tolist()):
        observers.setdefault(o[0], set()).add(o[1])
        lev[o] = l
    # w(i, j) = the number of points whose observer set holds both (points with the same set are added together)
    W = np.zeros((nk, nk), np.int64)
    for s, points in collections.Counter(frozenset(s) for s in observers.values()).items():
        if len(s) == 2:                                      # (the same statement as below, without numpy's set-up cost)
            i, j = s
            W[i, j] += points
            W[j, i] += points
        else:
            a = np.array(sorted(s))
            W[np.ix_(a, a)] += points
    np.fill_diagonal(W, 0)
    for i in range(nk):
        w = W[i]
        q = np.nonzero(w >= min_weight)[0]
        if len(q) == 0 and w.max() > 0:
            q = np.array([int(np.argmax(w))])                # the fallback: the largest weight, the smallest index on a tie
        q = q[np.lexsort((q, -w[q]))]                        # weight descending, index ascending on equal weight
        m = min(len(q), nbs)
        out["nb_count"][i], out["nb_idx"][i, :m], out["nb_weight"][i, :m] = len(q), q[:m], w[q[:m]]
        if i > 0 and w[:i].max() > 0:
            out["parent"][i] = int(np.argmax(w[:i]))         # the earlier key frame with the largest weight, the first of them
    # the culling statistic.  A subject's level passes its own test (slack >= 0), so among the point's sorted levels the
    # observers that count are those at or below level + slack, less the subject itself.
    levels = {p: sorted(lev[p, o] for o in s) for p, s in observers.items()}
    for (p, k), subject in zip(obs, [1] * count if mask is None else mask[:count].tolist()):
        if not subject:
            continue
        out["kf_points"][k] += 1
        if bisect.bisect_right(levels[p], lev[p, k] + slack) - 1 >= min_observers:
            out["kf_redundant"][k] += 1
    return out


def ref_batch(bt, prm, nbs):
    maps = [ref_map(bt["pt"][b], bt["kf"][b], None if bt["level"] is None else bt["level"][b],
                    None if bt["mask"] is None else bt["mask"][b], int(bt["counts"][b]), int(bt["nk"][b]), bt["ks"], prm, nbs)
            for b in range(len(bt["counts"]))]
    return {k: np.stack([np.asarray(m[k]) for m in maps]) for k in NAMES}


def assert_same(got, want, what):
    for k in NAMES:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not (g == w).all():
            at = tuple(int(v[0]) for v in np.nonzero(g != w))
            raise AssertionError("%s: %s differs at %r: %d against %d" % (what, k, at, g[at], w[at]))


# ---- maps -----------------------------------------------------------------------------------------------------------------
def make_map(points, nk, rng=None, levels=False, mask=False):
    """A map from {point: observers}: the sorted list, with random levels 0..7 and a random mask if asked for."""
    obs = sorted((p, k) for p, s in points.items() for k in s)
    n = len(obs)
    m = dict(pt=np.array([o[0] for o in obs], np.int32).reshape(n), kf=np.array([o[1] for o in obs], np.uint16).reshape(n), nk=nk)
    if levels:
        m["level"] = rng.integers(0, 8, n).astype(np.uint8)
    if mask:
        m["mask"] = (rng.random(n) < 0.7).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    return m


def random_map(seed, nk, extra=0):
    """Point p has 1 + p mod nk observers, so every observer count from 1 to nk occurs; nk == 0: no observation."""
    rng = np.random.default_rng(seed)
    points = {3 * p + 1: set(rng.choice(nk, 1 + p % nk, replace=False).tolist()) for p in range(nk + extra if nk else 0)}
    return make_map(points, nk, rng, levels=True, mask=True)


def pairs_map(nk, shared=1, spare=0):
    """Every pair of the first nk key frames shares `shared` points of its own; `spare` key frames observe nothing."""
    points, p = {}, 0
    for i in range(nk):
        for j in range(i + 1, nk):
            for _ in range(shared):
                points[p] = {i, j}
                p += 1
    return make_map(points, nk + spare)


def clique_map(nk, shared):
    """`shared` points that every key frame observes."""
    return make_map({p: set(range(nk)) for p in range(shared)}, nk)


def path_map(seed, nk, points=600, run=6):
    """Key frames along a path: each point is seen by a run of consecutive key frames."""
    rng = np.random.default_rng(seed)
    out = {}
    for p in range(points):
        a = int(rng.integers(0, nk - 1))
        out[p] = set(range(a, min(nk, a + int(rng.integers(2, run + 1)))))
    return make_map(out, nk, rng, levels=True)


def batch_of(maps, pad=(0, 0), seed=99, level=None, mask=None, stride=None):
    """The maps as one batch.  A map is dict(pt, kf, nk[, level][, mask][, count]); count defaults to the list's length
    and may lie.  Strides: the largest list / nk plus `pad`, at least 1, or the observation stride given."""
    rng = np.random.default_rng(seed)
    B = len(maps)
    S = stride or max(max(len(m["pt"]) for m in maps) + pad[0], 1)
    ks = max(max(m.get("ks", m["nk"]) for m in maps) + pad[1], 1)
    level = any("level" in m for m in maps) if level is None else level
    mask = any("mask" in m for m in maps) if mask is None else mask
    bt = dict(pt=rng.integers(-2 ** 31, 2 ** 31, (B, S)).astype(np.int32), kf=rng.integers(0, 1 << 16, (B, S)).astype(np.uint16),
              level=rng.integers(0, 256, (B, S)).astype(np.uint8) if level else None,
              mask=rng.integers(0, 256, (B, S)).astype(np.uint8) if mask else None,
              counts=np.zeros(B, np.int32), nk=np.zeros(B, np.int32), ks=ks)
    for b, m in enumerate(maps):
        n = len(m["pt"])
        bt["pt"][b, :n], bt["kf"][b, :n] = m["pt"], m["kf"]
        if level:
            bt["level"][b, :n] = m.get("level", 0)           # (no levels: all zero)
        if mask:
            bt["mask"][b, :n] = m.get("mask", 1)             # (no mask: all count)
        bt["counts"][b], bt["nk"][b] = m.get("count", n), m["nk"]
    return bt


def edit(m, **kw):
    out = dict(m)
    out.update(kw)
    return out


# ---- the case list ----------------------------------------------------------------------------------------------------------
MIXED_NK = (0, 1, 2, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def mixed_batch():
    return batch_of([random_map(10 + nk, nk, extra=nk // 3) for nk in MIXED_NK], pad=(5, 3))


def tie_maps():
    quiet = random_map(5, 12)                   # 12 key frames, 12 points: nobody comes near 15 shared points
    return [pairs_map(9, 1), pairs_map(6, 2, spare=2), edit(quiet, nk=14), clique_map(5, 3)]


def culling_maps():
    """Point 0: levels 2, 3, 3, 4, 4, 5 seen from key frames 0..5.  With slack 0 the subject at level 4 has exactly 4
    others at or below 4 (and the other level-4 observer decides at equality); with slack 1 the subject at level 3 gains
    the two at level 4.  Points 1 and 2 give the same subject 3 and 2 others: min_observers met exactly, missed by one."""
    lv = {0: [2, 3, 3, 4, 4, 5], 1: [1, 1, 1, 1], 2: [1, 1, 1], 3: [0, 7], 4: [6]}
    points = {p: set(range(len(v))) for p, v in lv.items()}
    m = make_map(points, 7)
    m["level"] = np.array([lv[p][k] for p, k in zip(m["pt"].tolist(), m["kf"].tolist())], np.uint8)
    masked = edit(m, mask=np.array([0 if (p + k) % 3 == 0 else 9 for p, k in zip(m["pt"].tolist(), m["kf"].tolist())], np.uint8))
    return [m, masked, random_map(77, 20, extra=30)]


CULLING_PARAMS = ((1, 3, 0), (1, 3, 1), (1, 4, 0), (1, 2, 1), (1, 1, 0), (1, 5, 255))


def malformed_maps():
    """(name, map): each breaks one rule of the list, the counts or the key-frame count."""
    g = random_map(31, 9, extra=6)
    n = len(g["pt"])
    at = next(i for i in range(1, n) if g["pt"][i] == g["pt"][i - 1])         # inside a point
    new = next(i for i in range(1, n) if g["pt"][i] != g["pt"][i - 1])        # the first observation of a point
    def put(name, i, v):
        a = g[name].copy()
        a[i] = v
        return {name: a}
    swap_kf = g["kf"].copy()
    swap_kf[[at - 1, at]] = swap_kf[[at, at - 1]]
    return [("equal consecutive pairs", edit(g, **put("kf", at, g["kf"][at - 1]))),
            ("a descending obs_kf within a point", edit(g, kf=swap_kf)),
            ("a descending obs_pt", edit(g, **put("pt", new, g["pt"][new - 1] - 1))),
            ("obs_kf == nk", edit(g, **put("kf", n - 1, 9))),
            ("a negative obs_pt", edit(g, **put("pt", 0, -1))),
            ("counts > stride", edit(g, count="stride + 1")),
            ("counts < 0", edit(g, count=-1)),
            ("nk > kf_stride", edit(g, nk="kf_stride + 1")),
            ("nk < 0", edit(g, nk=-2))]


def malformed_batch(bad):
    """The faulty map between two good ones, with strides that leave room behind every list."""
    good = [random_map(41, 11, extra=8), random_map(42, 7, extra=20)]
    bt = batch_of([good[0], edit(bad, count=0 if isinstance(bad.get("count"), str) else bad.get("count", len(bad["pt"])),
                                 nk=0 if isinstance(bad["nk"], str) else bad["nk"], ks=9), good[1]], pad=(4, 2))
    if bad.get("count") == "stride + 1":
        bt["counts"][1] = bt["pt"].shape[1] + 1
    if bad["nk"] == "kf_stride + 1":
        bt["nk"][1] = bt["ks"] + 1
    return bt


@functools.lru_cache(maxsize=None)
def limit_batch():
    """nk = kf_stride = 4096: one point that all 4096 key frames observe, 70 000 points that the pair (100, 200) shares (a
    weight beyond 16 bits), 2 points each that key frame 7 shares with key frames 1000..3199 (with min_weight 2 its row
    holds 2200 neighbours and more: the sort runs 4096 wide), and random points."""
    rng = np.random.default_rng(4096)
    points = {0: set(range(4096))}
    p = 1
    for _ in range(70000):
        points[p] = {100, 200}
        p += 1
    for j in range(1000, 3200):
        for _ in range(2):
            points[p] = {7, j}
            p += 1
    for _ in range(3000):
        points[p] = set(rng.choice(4096, int(rng.integers(1, 7)), replace=False).tolist())
        p += 1
    return batch_of([make_map(points, 4096, rng, levels=True, mask=True)])


LIMIT_PARAMS, LIMIT_NBS = (2, 3, 1), 64


# One map for three passes of both grids: the count kernel walks batch * stride slots, CV_THREADS * CV_GRID_CAP a pass, so
# 2 * 262144 + 1 = 524289 slots (all of them observations) make three; the row kernel walks batch * kf_stride rows,
# CV_GRID_CAP a pass, so 2 * 1024 + 1 = 2049 rows make three.
PASS_SLOTS, PASS_ROWS = 2 * CV_THREADS * CV_GRID_CAP + 1, 2 * CV_GRID_CAP + 1


@functools.lru_cache(maxsize=None)
def passes_batch():
    rng = np.random.default_rng(2049)
    a = rng.integers(0, PASS_ROWS, PASS_SLOTS // 2 + 1)
    b = (a + 1 + rng.integers(0, 40, len(a)) ** 2 % (PASS_ROWS - 1)) % PASS_ROWS                  # (never a itself)
    pt = np.repeat(np.arange(len(a), dtype=np.int32), 2)
    kf = np.stack([np.minimum(a, b), np.maximum(a, b)], 1).reshape(-1).astype(np.uint16)
    m = dict(pt=pt[:PASS_SLOTS], kf=kf[:PASS_SLOTS], nk=PASS_ROWS, level=rng.integers(0, 4, PASS_SLOTS).astype(np.uint8))
    bt = batch_of([m])
    assert bt["pt"].shape == (1, PASS_SLOTS) and bt["ks"] == PASS_ROWS
    return bt


def tiny_variants():
    """2 key frames, 3 observations: a good map, a map with two points only, an empty one and a malformed one."""
    t = lambda pt, kf, **kw: dict(pt=np.array(pt, np.int32), kf=np.array(kf, np.uint16), nk=2, **kw)
    return [t([4, 4, 9], [0, 1, 1]), t([0, 1, 1], [1, 0, 1]), t([4, 4, 9], [0, 1, 1], count=0), t([4, 4, 4], [0, 1, 1])]


def case_list():
    """(name, batch, params, nb_stride) of everything but the limit case."""
    out = [("mixed min_weight %d" % w, mixed_batch(), (w, 3, 1), 40) for w in (1, 3, 15)]
    ties = batch_of(tie_maps(), pad=(2, 1))
    out += [("ties", ties, ORB, 5), ("ties, every link", ties, (1, 3, 1), ties["ks"])]
    out += [("truncation, nb_stride 3", batch_of([clique_map(8, 2), random_map(3, 30, extra=60)]), (1, 3, 1), 3),
            ("truncation, nb_stride nk - 1", batch_of([clique_map(17, 4)]), (4, 3, 1), 16)]
    cull = batch_of(culling_maps())
    out += [("culling %r" % (p,), cull, p, 4) for p in CULLING_PARAMS]
    out += [("culling without levels", edit(cull, level=None), (1, 3, 1), 4),
            ("culling with zero levels", edit(cull, level=np.zeros_like(cull["level"])), (1, 3, 1), 4)]
    out += [("malformed: " + name, malformed_batch(m), (2, 2, 1), 6) for name, m in malformed_maps()]
    out += [("tiny", batch_of(tiny_variants()), (1, 1, 0), 1)]
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's result of a named case, computed once."""
    if name == "limit":
        return ref_batch(limit_batch(), LIMIT_PARAMS, LIMIT_NBS)
    if name == "passes":
        return ref_batch(passes_batch(), (2, 1, 0), 8)
    _, bt, prm, nbs = next(c for c in case_list() if c[0] == name)
    return ref_batch(bt, prm, nbs)


# ---- the host probe -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probe_exe():
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(tempfile.mkdtemp(prefix="covis_probe_"), "covis_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", "covis_host_check.cpp"), "-o", exe])
    return exe


def probe(bt, prm, nbs):
    """The probe's result for a batch."""
    B, S = bt["pt"].shape
    ks = bt["ks"]
    words = [np.array([B], np.int32)]
    for b in range(B):
        words.append(np.array(list(prm) + [bt["nk"][b], ks, bt["counts"][b], S, nbs, bt["level"] is not None,
                                          bt["mask"] is not None], np.int32))
        words += [bt["pt"][b], bt["kf"][b].astype(np.int32)]
        words += [bt[k][b].astype(np.int32) for k in ("level", "mask") if bt[k] is not None]
    with tempfile.TemporaryDirectory(prefix="covis_case_") as d:
        np.concatenate(words).astype("<i4").tofile(os.path.join(d, "in.bin"))
        subprocess.run([probe_exe(), os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], check=True)
        w = np.fromfile(os.path.join(d, "out.bin"), "<i4").astype(np.int64).reshape(B, 1 + 4 * ks + 2 * ks * nbs)
    row = lambda i: w[:, 1 + i * ks:1 + (i + 1) * ks]
    idx = w[:, 1 + 4 * ks:1 + 4 * ks + ks * nbs].reshape(B, ks, nbs)
    return dict(status=w[:, 0], nb_count=row(0), parent=row(1), kf_points=row(2), kf_redundant=row(3),
                nb_idx=np.where(idx == SENT32, SENT16, idx), nb_weight=w[:, 1 + 4 * ks + ks * nbs:].reshape(B, ks, nbs))


@functools.lru_cache(maxsize=None)
def probe_limit():
    return probe(limit_batch(), LIMIT_PARAMS, LIMIT_NBS)


# ---- CPU tests ------------------------------------------------------------------------------------------------------------
def test_covisibility_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {}
    for f in ("pislam_covisibility_batch", "pislam_covisibility_reserve"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % f, code)
        assert m, f
        counts[f] = len(m.group(1).split(","))
    m = re.search(r"typedef struct pislam_covis_params \{([^}]*)\} pislam_covis_params;", code)
    assert m, "pislam_covis_params is not declared"
    fields = re.findall(r"(int32_t)\s+(\w+)\s*;", m.group(1))
    assert [f[1] for f in fields] == ["min_weight", "cull_min_observers", "cull_level_slack"]
    assert "#define PISLAM_ABI_VERSION 2" in text
    from pislam_amd import capi, frontend
    assert counts == {"pislam_covisibility_batch": 19, "pislam_covisibility_reserve": 4}
    for f, n in counts.items():
        assert len(capi.SYMBOLS[f][1]) == n, f
    assert [f[0] for f in capi.CovisParams._fields_] == [f[1] for f in fields] and ctypes.sizeof(capi.CovisParams) == 12
    for f in ("mapObservations", "reserveCovisibility", "covisibilityBatch", "essentialPairs"):
        assert callable(getattr(frontend, f))
    assert frontend.COVIS_MAX_KF == frontend.POSE_GRAPH_MAX_VERTICES == 4096
    lib = capi.load()
    for f in counts:
        assert hasattr(lib, f)
    assert "covis_host_check.cpp" in open(os.path.join(ROOT, "tools", "probes", "README.md")).read()
    kernels = open(os.path.join(ROOT, "pislam_amd", "csrc", "pislam_covis_kernels.h")).read()
    assert "CV_THREADS = %d;" % CV_THREADS in kernels and "CV_GRID_CAP = %d;" % CV_GRID_CAP in kernels


def test_covisibility_cases_cover_what_they_are_meant_to():
    """The restatement's own results show that the cases reach the paths they are named after."""
    r = reference("mixed min_weight 15")
    assert r["status"].tolist() == [1, 0, 0, 0, 0, 0, 0] and (r["nb_count"][6] > 0).any()
    assert r["parent"][:, 0].tolist() == [NO_PARENT] * 7
    t = reference("ties")
    assert (t["nb_count"][0, :9] == 1).all() and t["nb_idx"][0, :9, 0].tolist() == [1] + [0] * 8      # the fallback and its tie
    assert t["parent"][0, :9].tolist() == [NO_PARENT] + [0] * 8
    assert t["nb_count"][1, 6:8].tolist() == [0, 0] and t["parent"][1, 6:8].tolist() == [NO_PARENT] * 2  # no observation at all
    e = reference("ties, every link")
    assert e["nb_idx"][0, 4, :8].tolist() == [0, 1, 2, 3, 5, 6, 7, 8]
    tr = reference("truncation, nb_stride 3")
    assert (tr["nb_count"][0, :8] == 7).all() and (tr["nb_idx"][0, :8] != SENT16).all()
    full = reference("truncation, nb_stride nk - 1")
    assert (full["nb_count"][0] == 16).all() and (full["nb_weight"][0] == 4).all()
    by = {p: reference("culling %r" % (p,)) for p in CULLING_PARAMS}
    # key frame 3 sees point 0 at level 4 (4 others at or below 4), point 1 at level 1 (3 others) and nothing else
    assert by[(1, 3, 0)]["kf_points"][0, 3] == 2 and by[(1, 3, 0)]["kf_redundant"][0, 3] == 2
    assert by[(1, 4, 0)]["kf_redundant"][0, 3] == 1 and by[(1, 5, 255)]["kf_redundant"][0, 3] == 1
    # key frame 1 sees point 0 at level 3: 2 others at or below 3, 4 at or below 4
    assert by[(1, 3, 0)]["kf_redundant"][0, 1] == 1 and by[(1, 3, 1)]["kf_redundant"][0, 1] == 2
    # key frame 2 sees point 2 with exactly 2 others: met exactly at 2, missed by one at 3
    assert by[(1, 2, 1)]["kf_redundant"][0, 2] == 3 and by[(1, 3, 1)]["kf_redundant"][0, 2] == 2
    assert (by[(1, 3, 1)]["kf_points"][1] < by[(1, 3, 1)]["kf_points"][0]).any()                   # the mask removes subjects ...
    assert (by[(1, 3, 1)]["nb_weight"][1] == by[(1, 3, 1)]["nb_weight"][0]).all()                  # ... and no observer
    assert_same(reference("culling without levels"), reference("culling with zero levels"), "levels")
    for name, _ in malformed_maps():
        m = reference("malformed: " + name)
        assert m["status"].tolist() == [0, 3, 0], name
        assert (m["nb_count"][1] == 0).all() and (m["parent"][1] == NO_PARENT).all() and (m["nb_idx"][1] == SENT16).all(), name
        assert (m["kf_points"][1] == 0).all() and (m["kf_redundant"][1] == 0).all(), name
    assert reference("tiny")["status"].tolist() == [0, 0, 1, 3]


def test_covisibility_probe_equals_the_restatement():
    for name, bt, prm, nbs in case_list():
        assert_same(probe(bt, prm, nbs), reference(name), name)


def test_covisibility_probe_equals_the_restatement_at_the_limit():
    want = reference("limit")
    assert_same(probe_limit(), want, "limit")
    assert want["nb_count"][0, 7] > 2048 and want["nb_weight"][0, 100, 0] == 70001 and want["nb_idx"][0, 100, 0] == 200
    assert (want["nb_count"][0] > LIMIT_NBS).any() and want["status"][0] == 0
    assert_same(probe(passes_batch(), (2, 1, 0), 8), reference("passes"), "passes")


def brute_pairs(r, b, nk, min_weight):
    tree = [(int(r["parent"][b, k]), k) for k in range(nk) if r["parent"][b, k] != NO_PARENT]
    links = set()
    for i in range(nk):
        for c in range(int(r["nb_count"][b, i])):
            if r["nb_weight"][b, i, c] >= min_weight:
                j = int(r["nb_idx"][b, i, c])
                links.add((min(i, j), max(i, j)))
    return tree + sorted(links - set(tree))


def as_tensors(r):
    import torch
    t = lambda k, dt: torch.from_numpy(np.asarray(r[k]).astype(dt))
    parent = torch.from_numpy(np.asarray(r["parent"]).astype(np.uint16).view(np.int16))
    return t("nb_idx", np.int16), t("nb_weight", np.int32), t("nb_count", np.int32), parent


def test_map_observations_sorts_every_list_alike():
    import torch
    from pislam_amd.frontend import mapObservations
    rng = np.random.default_rng(8)
    B, S = 3, 50
    counts = np.array([50, 17, 0], np.int32)
    kf, pt = rng.integers(0, 4096, (B, S)).astype(np.int16), rng.integers(0, 9, (B, S)).astype(np.int32)
    level, words = rng.integers(0, 8, (B, S)).astype(np.uint8), rng.integers(0, 1 << 30, (B, S, 2)).astype(np.int32)
    out = mapObservations(*(torch.from_numpy(a) for a in (kf, pt, counts, level, words)))
    assert [o.dtype for o in out] == [torch.int16, torch.int32, torch.int32, torch.uint8, torch.int32]
    okf, opt, ocounts, olevel, owords = (o.numpy() for o in out)
    assert ocounts.tolist() == counts.tolist()
    for b in range(B):
        n = counts[b]
        order = sorted(range(n), key=lambda i: (pt[b, i], kf[b, i], i)) + list(range(n, S))
        for got, src in ((okf, kf), (opt, pt), (olevel, level), (owords, words)):
            assert (got[b] == src[b][order]).all()
    # counts beyond the stride and below zero are clamped
    assert mapObservations(torch.from_numpy(kf), torch.from_numpy(pt), torch.tensor([99, -4, 3]))[2].tolist() == [50, 0, 3]
    with pytest.raises(ValueError, match="further tensor"):
        mapObservations(torch.from_numpy(kf), torch.from_numpy(pt), torch.from_numpy(counts), torch.zeros(B, S + 1))


def test_essential_pairs_tree_first_then_every_strong_link_once():
    import torch
    from pislam_amd.frontend import essentialGraph, essentialPairs
    bt = batch_of([path_map(1, 40), random_map(2, 25, extra=200), clique_map(6, 9)])
    r = ref_batch(bt, (3, 3, 1), bt["ks"])
    nk = torch.from_numpy(bt["nk"])
    for min_weight in (3, 5, 100):
        got = essentialPairs(*as_tensors(r), nk, min_weight=min_weight)
        assert len(got) == 3
        for b in range(3):
            want = brute_pairs(r, b, int(bt["nk"][b]), min_weight)
            assert got[b].dtype == torch.int32 and got[b].tolist() == [list(p) for p in want], (min_weight, b)
    want = brute_pairs(r, 0, 40, 3)
    assert [p[1] for p in want[:39]] == list(range(1, 40)) and len(want) > 60 and all(i < j for i, j in want)
    assert len(set(want)) == len(want) and want[39:] == sorted(want[39:])
    # a truncated row that may hide a strong link is refused; one whose last weight is below min_weight hides none
    cut = ref_batch(bt, (3, 3, 1), 2)
    assert (cut["nb_count"] > 2).any()
    with pytest.raises(ValueError, match="truncated"):
        essentialPairs(*as_tensors(cut), nk, min_weight=3)
    top = int(cut["nb_weight"][cut["nb_count"] > 2][:, 1].max())
    assert [g.tolist() for g in essentialPairs(*as_tensors(cut), nk, min_weight=top + 1)] == \
        [[list(p) for p in brute_pairs(r, b, int(bt["nk"][b]), top + 1)] for b in range(3)]
    # through essentialGraph: per vertex ascending entries, and the index ends at 2 * ne
    pairs = essentialPairs(*as_tensors(r), nk, min_weight=5)
    path = torch.tensor([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1 * k, 0, 0, 1] for k in range(40)], dtype=torch.float32)
    sims = [path, path[:25], path[:6]]
    fixed = [torch.zeros(int(n), dtype=torch.uint8) for n in bt["nk"]]
    _, v_counts, _, edges, _, _, e_counts, inc_ptr, inc = essentialGraph(sims, fixed, pairs)
    for b in range(3):
        ne, nv = int(e_counts[b]), int(v_counts[b])
        assert ne == len(pairs[b]) and edges[b, :ne].tolist() == pairs[b].tolist()
        ptr, ent = inc_ptr[b].tolist(), inc[b].tolist()
        assert ptr[0] == 0 and ptr[nv] == 2 * ne
        for k in range(nv):
            mine = ent[ptr[k]:ptr[k + 1]]
            assert mine == sorted(set(mine)) and all(edges[b, e >> 1, e & 1] == k for e in mine)


class Recorder:
    """The stand-in for a Context, as in test_backend_wrappers.py: nothing behind it."""

    class _Lib:
        def __init__(self, calls):
            self._calls = calls

        def __getattr__(self, name):
            def record(*args):
                self._calls.append([name, args])
                return 0
            return record

    def __init__(self):
        self.h = object()
        self.calls, self.checked = [], []
        self.lib = self._Lib(self.calls)

    def check(self, rc, what):
        self.checked.append(what)


def test_covisibility_wrapper_refuses_with_its_messages():
    import torch
    from pislam_amd.frontend import covisibilityBatch
    B, S, KS, NB = 2, 8, 5, 3
    z = lambda dt, *shape: torch.zeros(shape, dtype=dt)
    strided = lambda t: torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype)[..., ::2]
    base = lambda: dict(obs_kf=z(torch.int16, B, S), obs_pt=z(torch.int32, B, S), counts=z(torch.int32, B),
                        kf_counts=z(torch.int32, B), kf_stride=KS, nb_stride=NB)
    ctx = Recorder()
    out = covisibilityBatch(**base(), ctx=ctx)
    assert [tuple(o.shape) for o in out] == [(B, KS, NB), (B, KS, NB), (B, KS), (B, KS), (B, KS), (B, KS), (B,)]
    assert [o.dtype for o in out] == [torch.int16, torch.int32, torch.int32, torch.int16, torch.int32, torch.int32, torch.int32]
    (name, args), = ctx.calls
    assert name == "pislam_covisibility_batch" and len(args) == 19 and ctx.checked == [name]
    assert args[6:12] == (0, 0, KS, S, NB, B) and bytes(args[1]._obj) == np.array(ORB, np.int32).tobytes()
    assert list(args[12:]) == [o.data_ptr() for o in out]
    # the strides taken from outputs that are passed; unsigned words
    ctx = Recorder()
    given = dict(nb_count=z(torch.int32, B, KS), nb_idx=z(torch.uint16, B, KS, NB), parent=z(torch.uint16, B, KS))
    out = covisibilityBatch(**dict(base(), kf_stride=None, nb_stride=None, obs_kf=z(torch.uint16, B, S)), **given,
                            obs_level=z(torch.uint8, B, S), cull_mask=z(torch.uint8, B, S), ctx=ctx)
    assert out[0] is given["nb_idx"] and out[2] is given["nb_count"] and out[3] is given["parent"]
    assert ctx.calls[0][1][8:12] == (KS, S, NB, B) and 0 not in ctx.calls[0][1][6:8]
    refused = {
        "obs_pt must be a 32-bit integer tensor [batch][stride]": [dict(obs_pt=z(torch.int64, B, S)), dict(obs_pt=z(torch.int32, B * S))],
        "obs_kf must be a 16-bit integer tensor [batch][stride]": [dict(obs_kf=z(torch.uint8, B, S)), dict(obs_kf=z(torch.int16, B, S + 1))],
        "counts and kf_counts must be 32-bit integer tensors [batch]": [dict(counts=z(torch.int64, B)), dict(kf_counts=z(torch.int32, B + 1))],
        "obs_level must be a uint8 tensor [batch][stride]": [dict(obs_level=z(torch.int32, B, S)), dict(obs_level=z(torch.uint8, B, S + 1))],
        "cull_mask must be a uint8 tensor [batch][stride]": [dict(cull_mask=z(torch.bool, B, S)), dict(cull_mask=z(torch.uint8, B + 1, S))],
        "kf_stride is needed, or the output nb_count [batch][kf_stride] to take it from": [dict(kf_stride=None)],
        "kf_stride must be 1..4096": [dict(kf_stride=0), dict(kf_stride=4097)],
        "nb_stride must be 1..kf_stride": [dict(nb_stride=0), dict(nb_stride=KS + 1)],
        "min_weight and cull_min_observers must be >= 1 and cull_level_slack 0..255":
            [dict(min_weight=0), dict(cull_min_observers=0), dict(cull_level_slack=-1), dict(cull_level_slack=256)],
        "nb_idx must be a 16-bit integer tensor [batch][kf_stride][nb_stride]": [dict(nb_idx=z(torch.int32, B, KS, NB)),
                                                                                 dict(nb_idx=z(torch.int16, B, KS, NB + 1))],
        "nb_weight must be a 32-bit integer tensor [batch][kf_stride][nb_stride]": [dict(nb_weight=z(torch.int64, B, KS, NB)),
                                                                                    dict(nb_weight=z(torch.int32, B, KS + 1, NB))],
        "parent must be a 16-bit integer tensor [batch][kf_stride]": [dict(parent=z(torch.int32, B, KS)), dict(parent=z(torch.int16, B, KS + 1))],
        "nb_count, kf_points and kf_redundant must be 32-bit integer tensors [batch][kf_stride]":
            [dict(nb_count=z(torch.int32, B, KS + 1)), dict(kf_points=z(torch.int64, B, KS)), dict(kf_redundant=z(torch.int32, B, KS, 1))],
        "status must be a 32-bit integer tensor [batch]": [dict(status=z(torch.int32, B + 1)), dict(status=z(torch.uint8, B))],
        "inputs must be contiguous": [dict(obs_pt=strided(z(torch.int32, B, S))), dict(cull_mask=strided(z(torch.uint8, B, S)))],
        "outputs must be contiguous": [dict(nb_weight=strided(z(torch.int32, B, KS, NB))), dict(status=strided(z(torch.int32, B)))],
    }
    for message, changes in refused.items():
        for change in changes:
            ctx = Recorder()
            with pytest.raises(ValueError) as e:
                covisibilityBatch(**dict(base(), **change), ctx=ctx)
            assert str(e.value) == message, change
            assert ctx.calls == [] and ctx.checked == []


# ---- GPU tests ------------------------------------------------------------------------------------------------------------
def device_inputs(bt):
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return dict(obs_kf=up(bt["kf"].view(np.int16)), obs_pt=up(bt["pt"]), counts=up(bt["counts"]), kf_counts=up(bt["nk"]),
                obs_level=up(bt["level"]), cull_mask=up(bt["mask"]))


def sentinels(B, ks, nbs):
    import torch
    f = lambda dt, *s: torch.full(s, 0x5A, dtype=torch.uint8, device="cuda").view(dt).reshape(*s[:-1], -1)
    return dict(nb_idx=f(torch.int16, B, ks, 2 * nbs), nb_weight=f(torch.int32, B, ks, 4 * nbs), nb_count=f(torch.int32, B, 4 * ks),
                parent=f(torch.int16, B, 2 * ks), kf_points=f(torch.int32, B, 4 * ks), kf_redundant=f(torch.int32, B, 4 * ks),
                status=f(torch.int32, 4 * B))


def result(outs):
    """The call's outputs as a RESULT: the 16-bit words unsigned."""
    r = {k: o.cpu().numpy().astype(np.int64) for k, o in zip(NAMES, outs)}
    r["nb_idx"], r["parent"] = r["nb_idx"] & 0xFFFF, r["parent"] & 0xFFFF
    return r


def gpu(ctx, bt, prm, nbs, inputs=None):
    from pislam_amd.frontend import covisibilityBatch
    o = sentinels(len(bt["counts"]), bt["ks"], nbs)
    outs = covisibilityBatch(**(inputs or device_inputs(bt)), kf_stride=bt["ks"], nb_stride=nbs, min_weight=prm[0],
                             cull_min_observers=prm[1], cull_level_slack=prm[2], **o, ctx=ctx)
    ctx.synchronize()
    assert all(a is b for a, b in zip(outs, o.values()))
    return result(outs)


def run_cases(gpu_ctx, prefix):
    ran = 0
    for name, bt, prm, nbs in case_list():
        if name.startswith(prefix):
            assert_same(gpu(gpu_ctx, bt, prm, nbs), reference(name), name)
            ran += 1
    assert ran


@pytest.mark.gpu
def test_covisibility_mixed_batch(gpu_ctx):
    run_cases(gpu_ctx, "mixed")


@pytest.mark.gpu
def test_covisibility_ties_fallback_and_empty_key_frames(gpu_ctx):
    run_cases(gpu_ctx, "ties")


@pytest.mark.gpu
def test_covisibility_truncated_rows_leave_the_rest_untouched(gpu_ctx):
    run_cases(gpu_ctx, "truncation")


@pytest.mark.gpu
def test_covisibility_culling_statistic(gpu_ctx):
    run_cases(gpu_ctx, "culling")


@pytest.mark.gpu
def test_covisibility_malformed_maps_between_good_ones(gpu_ctx):
    run_cases(gpu_ctx, "malformed")
    run_cases(gpu_ctx, "tiny")


@pytest.mark.gpu
def test_covisibility_at_the_limit(gpu_ctx):
    """kf_stride = 4096 against the probe, which test_covisibility_probe_equals_the_restatement_at_the_limit pins."""
    assert_same(gpu(gpu_ctx, limit_batch(), LIMIT_PARAMS, LIMIT_NBS), probe_limit(), "limit")


@pytest.mark.gpu
def test_covisibility_numpy_inputs_equal_tensor_inputs(gpu_ctx):
    bt = mixed_batch()
    arrays = dict(obs_kf=bt["kf"].view(np.int16), obs_pt=bt["pt"], counts=bt["counts"], kf_counts=bt["nk"], obs_level=bt["level"],
                  cull_mask=bt["mask"])
    assert_same(gpu(gpu_ctx, bt, (3, 3, 1), 40, inputs=arrays), reference("mixed min_weight 3"), "numpy inputs")


@pytest.mark.gpu
def test_covisibility_host_refusals_write_nothing(gpu_ctx):
    """Parameters, strides, pointers and overlaps that the contract excludes give PISLAM_ERR_INVALID with a message before
    anything is written; batch 0 is a no-op; a workspace the device cannot hold is PISLAM_ERR_NOMEM."""
    import torch
    from pislam_amd import capi
    bt = batch_of(tie_maps(), pad=(2, 1))
    B, S, ks, nbs = len(bt["counts"]), bt["pt"].shape[1], bt["ks"], 5       # the shape of the case "ties"
    d, o = device_inputs(bt), sentinels(B, ks, nbs)
    lib, h, ptr = gpu_ctx.lib, gpu_ctx.h, capi.ptr

    def call(prm=ORB, shape=(ks, S, nbs), batch=B, **repl):
        t = dict(d, **o)
        t.update(repl)
        p = None if prm is None else ctypes.byref(capi.CovisParams(*prm))
        return lib.pislam_covisibility_batch(h, p, ptr(t["obs_kf"]), ptr(t["obs_pt"]), ptr(t["counts"]), ptr(t["kf_counts"]),
                                             ptr(t["obs_level"]), ptr(t["cull_mask"]), shape[0], shape[1], shape[2], batch,
                                             *(ptr(t[k]) for k in NAMES))
    for prm in ((0, 3, 1), (-5, 3, 1), (15, 0, 1), (15, 3, -1), (15, 3, 256), None):
        assert call(prm=prm) == -1 and lib.pislam_last_error(h), prm
    for shape in ((0, S, 1), (4097, S, nbs), (ks, 0, nbs), (ks, 1 << 31, nbs), (ks, S, 0), (ks, S, ks + 1)):
        assert call(shape=shape) == -1, shape
    for bad in ((0, S), (4097, S), (ks, 0), (ks, 1 << 31)):
        assert lib.pislam_covisibility_reserve(h, bad[0], bad[1], B) == -1, bad
    assert call(batch=-1) == -1 and lib.pislam_covisibility_reserve(h, ks, S, -1) == -1
    host = np.zeros(B * ks * nbs + B * S, np.int32)
    for name in ("obs_kf", "obs_pt", "counts", "kf_counts") + NAMES:
        assert call(**{name: None}) == -1 and call(**{name: host}) == -1, name
    level = torch.zeros((B, S), dtype=torch.uint8, device="cuda")
    assert call(obs_level=host) == -1 and call(cull_mask=host) == -1
    assert call(status=d["counts"]) == -1 and call(nb_weight=d["obs_pt"]) == -1 and call(kf_points=level, obs_level=level) == -1
    assert call(nb_count=o["kf_points"]) == -1 and call(parent=o["nb_idx"].view(-1)[ks:]) == -1
    gpu_ctx.synchronize()
    for k, v in o.items():
        assert (v.cpu().numpy().view(np.uint8) == 0x5A).all(), k
    assert lib.pislam_covisibility_batch(h, ctypes.byref(capi.CovisParams(*ORB)), *([None] * 6), ks, S, nbs, 0, *([None] * 7)) == 0
    assert lib.pislam_covisibility_reserve(h, ks, S, 0) == 0
    assert call(obs_level=level, cull_mask=None) == 0 and call() == 0              # the optional inputs alone may be null
    gpu_ctx.synchronize()
    assert_same(result(o.values()), reference("ties"), "after the refusals")
    fresh = capi.Context(device=0, stream=torch.cuda.current_stream().cuda_stream)
    try:                                                     # 2^57 bytes: refused at once, nothing is allocated
        assert fresh.lib.pislam_covisibility_reserve(fresh.h, 4096, S, 2 ** 31 - 1) == -3
        assert fresh.lib.pislam_covisibility_reserve(fresh.h, ks, S, B) == 0
    finally:
        fresh.close()


@pytest.mark.gpu
def test_covisibility_small_call_after_a_large_one_on_the_same_workspace():
    """A context of its own, reserved once for the larger shape: the second call must not see the first one's matrix."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import reserveCovisibility
    big, small = mixed_batch(), batch_of(tie_maps(), pad=(2, 1))
    ctx = Context(device=0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        reserveCovisibility(big["ks"], big["pt"].shape[1], len(big["counts"]), ctx=ctx)
        assert_same(gpu(ctx, big, (1, 3, 1), 40), reference("mixed min_weight 1"), "the large call")
        assert_same(gpu(ctx, small, (1, 3, 1), small["ks"]), reference("ties, every link"), "the small call after it")
        assert_same(gpu(ctx, big, (15, 3, 1), 40), reference("mixed min_weight 15"), "the large call again")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_covisibility_many_tiny_maps_walk_the_row_grid_in_passes(gpu_ctx):
    """65 537 maps of 2 key frames and 3 observation slots: 131 074 rows are 129 passes of the row kernel's CV_GRID_CAP
    workgroups.  Map b is variant b mod 4 of the tiny case, so the restatement is that case's, repeated."""
    B = 65537
    four = batch_of(tiny_variants())
    pick = np.arange(B) % 4
    bt = dict(four, pt=four["pt"][pick], kf=four["kf"][pick], counts=four["counts"][pick], nk=four["nk"][pick])
    assert B * bt["ks"] > 3 * CV_GRID_CAP and B > 65535
    want = {k: v[pick] for k, v in reference("tiny").items()}
    assert_same(gpu(gpu_ctx, bt, (1, 1, 0), 1), want, "65537 tiny maps")


@pytest.mark.gpu
def test_covisibility_one_map_walks_both_grids_in_three_passes(gpu_ctx):
    bt = passes_batch()
    assert bt["pt"].size > 2 * CV_THREADS * CV_GRID_CAP and int(bt["counts"][0]) == bt["pt"].size
    assert int(bt["nk"][0]) > 2 * CV_GRID_CAP
    assert_same(gpu(gpu_ctx, bt, (2, 1, 0), 8), reference("passes"), "three passes")


@pytest.mark.gpu
def test_covisibility_graph_replay_on_changed_inputs(gpu_ctx):
    """After reserveCovisibility on a fresh context the call is captured on a side stream without a warm-up call; two
    replays on inputs rewritten in place give the restatement's words each time."""
    import torch as t
    from pislam_amd.capi import Context
    from pislam_amd.frontend import covisibilityBatch, reserveCovisibility
    first = batch_of([random_map(61, 20, extra=30), random_map(62, 33, extra=10)], stride=900)
    second = batch_of([random_map(63, 33, extra=25), random_map(64, 9, extra=3)], stride=900, seed=5)
    assert first["pt"].shape == second["pt"].shape and first["ks"] == second["ks"] == 33
    prm, nbs, B = (2, 3, 1), 7, 2
    gpu_ctx.synchronize()
    t.cuda.synchronize()
    side = t.cuda.Stream(t.device("cuda:0"))
    with t.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        reserveCovisibility(33, first["pt"].shape[1], B, ctx=ctx)
        d = device_inputs(first)
        o = sentinels(B, 33, nbs)
        side.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=side):
            covisibilityBatch(**d, kf_stride=33, nb_stride=nbs, min_weight=prm[0], cull_min_observers=prm[1],
                              cull_level_slack=prm[2], **o, ctx=ctx)
        for bt in (first, second):
            for k, v in device_inputs(bt).items():
                d[k].copy_(v)
            for x in o.values():
                x.view(t.uint8).fill_(0x5A)
            g.replay()
            side.synchronize()
            assert_same(result(o.values()), ref_batch(bt, prm, nbs), "replay")
        ctx.close()


@pytest.mark.gpu
def test_covisibility_chain_into_the_pose_graph(gpu_ctx):
    """40 key frames along a path: covisibilityBatch -> essentialPairs -> essentialGraph -> poseGraphBatch returns code 0,
    so the produced graph is connected and well formed for the call it feeds."""
    import torch
    from pislam_amd.frontend import (covisibilityBatch, essentialGraph, essentialPairs, mapObservations, poseGraphBatch,
                                     relativeSim3)
    m = path_map(7, 40)
    rng = np.random.default_rng(3)
    shuffle = rng.permutation(len(m["pt"]))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    kf, pt, counts, level = mapObservations(up(m["kf"].astype(np.int16)[shuffle][None]), up(m["pt"][shuffle][None]),
                                            up(np.array([len(shuffle)], np.int32)), up(m["level"][shuffle][None]))
    assert kf.cpu().numpy().view(np.uint16)[0].tolist() == m["kf"].tolist() and level.cpu().numpy()[0].tolist() == m["level"].tolist()
    nk = up(np.array([40], np.int32))
    outs = covisibilityBatch(kf, pt, counts, nk, obs_level=level, kf_stride=40, min_weight=15, **sentinels(1, 40, 40), ctx=gpu_ctx)
    gpu_ctx.synchronize()
    bt = batch_of([m])
    assert_same(result(outs), ref_batch(bt, ORB, 40), "path")
    pairs = essentialPairs(*outs[:4], nk, min_weight=30)
    assert pairs[0][:39, 1].tolist() == list(range(1, 40)) and len(pairs[0]) > 39
    sims = np.zeros((40, 13), np.float32)
    sims[:, [0, 4, 8, 12]] = 1.0
    sims[:, 9] = 0.3 * np.arange(40) + rng.normal(0, 0.01, 40)
    sims = up(sims)
    loop = relativeSim3(sims[0:1], sims[39:40])
    loop[0, 9] += 0.05                                       # the loop edge disagrees with the drifted chain
    with_loop = torch.cat([pairs[0], torch.tensor([[0, 39]], dtype=torch.int32, device="cuda")])
    fixed = torch.zeros(40, dtype=torch.uint8, device="cuda")
    fixed[0] = 1
    graph = essentialGraph(sims, fixed, with_loop, meas=loop)
    sims_out, cost, status = poseGraphBatch(*graph, ctx=gpu_ctx)
    gpu_ctx.synchronize()
    assert int(status[0]) & 255 == 0 and int(status[0]) >> 8 >= 2 and float(cost[0]) < 0.05 ** 2
