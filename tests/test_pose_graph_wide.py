"""pislam_pose_graph_wide_batch: the essential-graph optimisation of pislam_pose_graph_batch as a fixed sequence of
launches over all edges and vertices of all graphs, for graphs of up to 65536 vertices and 2^20 edges.

The contract is the comment of pislam_pose_graph_batch, so the expectation is the same everywhere: the host probe
(pgr::host_graph, which tests/test_pose_graph.py pins to its numpy restatement) word for word, on sims_out, cost, status
and the new work output (the solves attempted, the conjugate-gradient iterations made); and, within the old limits,
pislam_pose_graph_batch on the same device buffers byte for byte.  tools/probes/graph_wide_host_check.cpp is the probe
with the new limits: graph_host_check's lines in and out, and a binary case file for graphs too large for a text line.
The generators, Device, probe, cases() and assert_graphs are those of tests/test_pose_graph.py; the seeded family is the
pose_graph row of tests/test_backend_fuzz.py."""
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

import test_backend_fuzz as tf
import test_pose_graph as tg
from test_pose_graph import (BIG, COUNT_INVALID, DEFAULT, EMPTY, F32, F64, MAX_E, MAX_V, PG_FIELDS, SENT, SMALL, Device, assert_graphs,
                             bits, boundary_graphs, cases, edit, graph, make_graph, probe, shape_of, two_vertices)

WIDE_MAX_V, WIDE_MAX_E = 65536, 1 << 20
WIDE_FUNCS = ("pislam_pose_graph_wide_reserve", "pislam_pose_graph_wide_batch")


# ---- the probe with the new limits ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_exe():
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(tempfile.mkdtemp(prefix="graph_wide_probe_"), "graph_wide_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", "graph_wide_host_check.cpp"), "-o", exe])
    return exe


def write_binary(path, graphs, prms):
    """The binary case file of graph_wide_host_check.cpp (its head comment is the layout)."""
    with open(path, "wb") as f:
        f.write(b"PGWCASE1")
        np.array([len(graphs)], np.uint32).tofile(f)
        for g, p in zip(graphs, prms):
            w = g.get("weight")
            np.array(p[:2], np.int32).tofile(f)
            np.array(p[2:], F64).tofile(f)
            np.array([w is not None, len(g["sims"]), len(g["edges"])], np.uint32).tofile(f)
            for a, dt in ((g["fixed"], np.uint8), (g["sims"], F32), (g["edges"], np.uint32), (g["meas"], F32), (w, F32),
                          (g["inc_ptr"], np.uint32), (g["inc"], np.uint32)):
                if a is not None:
                    np.ascontiguousarray(a, dt).tofile(f)


def wide_lines(graphs, prms, binary=False):
    """The new probe's result lines for the graphs, from text lines or from a binary case file."""
    with tempfile.NamedTemporaryFile("w", suffix=".bin" if binary else ".txt", delete=False) as f:
        if not binary:
            f.write("\n".join(tg.case_line(g, p) for g, p in zip(graphs, prms)) + "\n")
    try:
        if binary:
            write_binary(f.name, graphs, prms)
        got = subprocess.run([wide_exe(), f.name], check=True, capture_output=True, text=True).stdout.splitlines()
    finally:
        os.unlink(f.name)
    assert len(got) == len(graphs)
    return got


def parse(g, ln):
    t = ln.split()
    nv = len(g["sims"])
    assert len(t) == 4 + 13 * nv
    return dict(status=int(t[0]), cost=float(np.array(int(t[1], 16), np.uint64).view(F64)), cg=int(t[2]), solves=int(t[3]),
                sims=np.array([int(x, 16) for x in t[4:]], np.uint32).view(F32).reshape(nv, 13))


def wide_probe(graphs, prms, binary=True):
    return [parse(g, ln) for g, ln in zip(graphs, wide_lines(graphs, prms, binary))]


# ---- graphs of this file ----------------------------------------------------------------------------------------------
PAST_PRM = (2, 8, 1e-3, 1e-9)


@functools.lru_cache(maxsize=None)
def past_the_old_limits():
    """One vertex and one edge more than pislam_pose_graph_batch takes; the graph of its limits test otherwise."""
    g = make_graph(31, nv=MAX_V + 1, extra=MAX_E - MAX_V, drift=0.01, span=40)
    assert shape_of([g]) == (MAX_V + 1, MAX_E + 1)
    return g


@functools.lru_cache(maxsize=None)
def past_the_old_limits_want():
    return wide_probe([past_the_old_limits()], [PAST_PRM])[0]


def rot_y(a):
    c, s, z, o = np.cos(a), np.sin(a), np.zeros_like(a), np.ones_like(a)
    return np.stack([c, z, s, z, o, z, -s, z, c], -1).reshape(-1, 3, 3)


def rot_z(a):
    c, s, z, o = np.cos(a), np.sin(a), np.zeros_like(a), np.ones_like(a)
    return np.stack([c, -s, z, s, c, z, z, z, o], -1).reshape(-1, 3, 3)


def pack13(R, t, s):
    return np.concatenate([R.reshape(-1, 9), t, s[:, None]], 1)


def mul_many(A, B):
    """A o B for rows of similarities, in binary64 (tg.sim_mul on arrays)."""
    Ra, Rb = A[:, :9].reshape(-1, 3, 3), B[:, :9].reshape(-1, 3, 3)
    return pack13(Ra @ Rb, A[:, 12:13] * np.einsum("nij,nj->ni", Ra, B[:, 9:12]) + A[:, 9:12], A[:, 12] * B[:, 12])


def rel_many(Si, Sj):
    """S_j o S_i^-1 for rows of similarities, in binary64 (tg.rel on arrays)."""
    Rt = Si[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
    return mul_many(Sj, pack13(Rt, -np.einsum("nij,nj->ni", Rt, Si[:, 9:12]) / Si[:, 12:13], 1.0 / Si[:, 12]))


@functools.lru_cache(maxsize=None)
def ring_with_chords(nv, ne, seed):
    """A ring of nv vertices and chords (k, k + m) for m = 2, 3, .. until there are ne edges, measured from the ground
    truth; every vertex but the fixed vertex 0 starts slightly off.  Vectorised: nothing here loops over an edge."""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(nv) / nv
    R = rot_y(a) @ rot_z(rng.normal(0, 0.05, nv))
    c = np.stack([4 * np.cos(a), 0.3 * rng.normal(size=nv), 4 * np.sin(a)], 1)
    s = np.exp(rng.normal(0, 0.05, nv))
    truth = pack13(R, -s[:, None] * np.einsum("nij,nj->ni", R, c), s)
    off = pack13(rot_z(rng.normal(0, 0.004, nv)), rng.normal(0, 0.02, (nv, 3)), np.exp(rng.normal(0, 0.004, nv)))
    off[0] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]
    est = mul_many(off, truth)
    k = np.arange(nv)
    edges = np.concatenate([np.stack([k, (k + m) % nv], 1) for m in range(1, ne // nv + 2)])[:ne]
    assert len(edges) == ne and (edges[:, 0] != edges[:, 1]).all()
    fixed = np.zeros(nv, np.uint8)
    fixed[0] = 1
    g = graph(est, fixed, edges, rel_many(truth[edges[:, 0]], truth[edges[:, 1]]))
    assert np.array_equal(g["sims"][0], truth[0].astype(F32))
    return g


# ---- CPU tests --------------------------------------------------------------------------------------------------------
def test_wide_call_is_declared_everywhere(tmp_path):
    header = os.path.join(ROOT, "include", "pislam_hip.h")
    text = open(header).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for f in WIDE_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % f, code), f
    m = re.search(r"int\s+pislam_pose_graph_wide_batch\s*\(([^)]*)\)", code)
    old = re.search(r"int\s+pislam_pose_graph_batch\s*\(([^)]*)\)", code)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]
    assert norm(m.group(1)) == norm(old.group(1)) + ["uint32_t *work"]       # the arguments of the old call, in its order
    assert re.search(r"Not here: a robust kernel, a several-workgroup form for one large graph\.\s+That form is a call of its own,"
                     r"[\s*]+pislam_pose_graph_wide_batch, below\.", text)
    assert "5 + iters * (5 + 6 * cg_iters)" in text
    cc = next((c for c in (os.environ.get("CC"), "gcc", "cc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "use.c"
    src.write_text('#include "pislam_hip.h"\nint (*wide)(pislam_ctx *, const pislam_pose_graph_params *, const float *, '
                   "const uint32_t *, const uint8_t *, const uint32_t *, const float *, const float *, const uint32_t *, "
                   "const uint32_t *, const uint32_t *, size_t, size_t, int, float *, double *, uint32_t *, uint32_t *) = "
                   "pislam_pose_graph_wide_batch;\nint (*reserve)(pislam_ctx *, size_t, size_t, int) = pislam_pose_graph_wide_reserve;\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(header), str(src)])
    from pislam_amd import capi, frontend
    assert len(capi.SYMBOLS["pislam_pose_graph_wide_batch"][1]) == 18 and len(capi.SYMBOLS["pislam_pose_graph_wide_reserve"][1]) == 4
    assert capi.SYMBOLS["pislam_pose_graph_wide_batch"][1][:17] == capi.SYMBOLS["pislam_pose_graph_batch"][1]
    assert (frontend.POSE_GRAPH_WIDE_MAX_VERTICES, frontend.POSE_GRAPH_WIDE_MAX_EDGES) == (WIDE_MAX_V, WIDE_MAX_E)
    assert (frontend.POSE_GRAPH_MAX_VERTICES, frontend.POSE_GRAPH_MAX_EDGES) == (MAX_V, MAX_E)
    for f in ("reservePoseGraphWide", "poseGraphWideBatch"):
        assert callable(getattr(frontend, f))
    lib = capi.load()
    for f in WIDE_FUNCS:
        assert hasattr(lib, f)
    assert "graph_wide_host_check.cpp" in open(os.path.join(ROOT, "tools", "probes", "README.md")).read()


def test_wide_probe_equals_the_old_probe_byte_for_byte():
    cs = cases()
    graphs = [g for _, g, _ in cs] + list(boundary_graphs())
    prms = [p for _, _, p in cs] + [BIG] * len(boundary_graphs())
    old = tg.run_probe([tg.case_line(g, p) for g, p in zip(graphs, prms)])
    assert wide_lines(graphs, prms) == old
    assert wide_lines(graphs, prms, binary=True) == old
    assert len({int(ln.split()[0]) & 255 for ln in old}) == 4 and any(int(ln.split()[2]) > 100 for ln in old)


def test_wide_probe_just_past_the_old_limits():
    g = past_the_old_limits()
    text, binary = wide_lines([g], [PAST_PRM]), wide_lines([g], [PAST_PRM], binary=True)
    assert text == binary
    want = parse(g, binary[0])
    assert want["status"] == 3 << 8 and want["cg"] == 16 and want["solves"] == 2 and bits(want["sims"]) != bits(g["sims"])
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write(tg.case_line(g, PAST_PRM) + "\n")
    try:
        r = subprocess.run([tg.probe_exe(), f.name], capture_output=True, text=True)
    finally:
        os.unlink(f.name)
    assert r.returncode == 2 and r.stdout == "" and "bad header" in r.stderr
    # and one vertex beyond the new limits is refused by the new probe
    r = subprocess.run([wide_exe()], input="G 1 1 0 0 0 %d 0\n" % (WIDE_MAX_V + 1), capture_output=True, text=True)
    assert r.returncode == 2 and "bad header" in r.stderr


def test_essential_graph_takes_the_wide_limits_when_asked():
    import torch
    from pislam_amd.frontend import essentialGraph
    sims = torch.zeros((3, 13), dtype=torch.float32)
    sims[:, [0, 4, 8, 12]] = 1.0
    fixed = torch.tensor([1, 0, 0], dtype=torch.uint8)
    pairs = torch.tensor([[0, 1], [1, 2], [0, 2]], dtype=torch.int32).repeat(5462, 1)[:MAX_E + 1]
    assert len(pairs) == MAX_E + 1
    with pytest.raises(ValueError) as e:
        essentialGraph(sims, fixed, pairs)
    assert str(e.value) == "at most 4096 vertices and 16384 edges per graph"
    with pytest.raises(ValueError) as e:
        essentialGraph(sims, fixed, pairs, wide=False)
    assert str(e.value) == "at most 4096 vertices and 16384 edges per graph"
    G = essentialGraph(sims, fixed, pairs, wide=True)
    assert tuple(G[3].shape) == (1, MAX_E + 1, 2) and G[6].tolist() == [MAX_E + 1] and tuple(G[8].shape) == (1, 2 * (MAX_E + 1))
    ptr, inc = tg.build_index(3, pairs.numpy())
    assert G[7][0].numpy().view(np.uint32).tolist() == ptr.tolist() and G[8][0].numpy().view(np.uint32).tolist() == inc.tolist()
    at = essentialGraph(sims, fixed, pairs[:MAX_E])                                  # the old limit itself still passes
    assert bits(at[4][0].numpy()) == bits(G[4][0, :MAX_E].numpy())
    big = torch.zeros((WIDE_MAX_V + 1, 13), dtype=torch.float32)
    with pytest.raises(ValueError) as e:
        essentialGraph(big, torch.zeros(WIDE_MAX_V + 1, dtype=torch.uint8), pairs[:3], wide=True)
    assert str(e.value) == "at most 65536 vertices and 1048576 edges per graph"


def wrapper_spec():
    """poseGraphBatch's cases in tests/test_backend_wrappers.py with the limits of the wide call, and the work output."""
    import test_backend_wrappers as tw
    spec = tw.W["poseGraphBatch"]
    good = dict(spec["good"])
    good["outputs-given"] = tw.put(sims_out=lambda: tw.z(tw.F32, tw.B, tw.V, 13), cost=lambda: tw.z(tw.F64, tw.B),
                                   status=lambda: tw.z(tw.I32, tw.B), work=lambda: tw.z(tw.I32, tw.B, 2))
    good["old-limits-passed"] = tw.both(tw.reshape("sims", 1, MAX_V + 1, 13), tw.reshape("fixed", 1, MAX_V + 1),
                                        tw.reshape("inc_ptr", 1, MAX_V + 2), tw.reshape("edges", 1, MAX_E + 1, 2),
                                        tw.reshape("meas", 1, MAX_E + 1, 13), tw.reshape("inc", 1, 2 * (MAX_E + 1)),
                                        tw.reshape("v_counts", 1), tw.reshape("e_counts", 1))
    refused = dict(spec["refused"])
    refused["vertex-limit"] = tw.reshape("sims", tw.B, WIDE_MAX_V + 1, 13)
    refused["edge-limit"] = tw.reshape("edges", tw.B, WIDE_MAX_E + 1, 2)
    return tw, spec["base"], good, refused


def run_wrapper(tw, base, change, refused):
    from pislam_amd import frontend as fe
    call = base()
    call.update(change(call))
    ctx = tw.Recorder()
    if refused:
        with pytest.raises(ValueError) as e:
            fe.poseGraphWideBatch(**call, ctx=ctx)
        assert ctx.calls == [] and ctx.checked == []
        return str(e.value)
    got = fe.poseGraphWideBatch(**call, ctx=ctx)
    named = {k: v for k, v in call.items() if hasattr(v, "data_ptr")}
    assert len(ctx.calls) == 1 and ctx.checked == ["pislam_pose_graph_wide_batch"] and len(got) == 4
    name, args = ctx.calls[0]
    return dict(fn=name, args=[tw._argument(a, ctx, named, got) for a in args],
                returns=[dict(dtype=str(t.dtype).replace("torch.", ""), shape=list(t.shape),
                              given=next((k for k, v in named.items() if v is t), None)) for t in got])


def test_wide_wrapper_refuses_as_the_old_wrapper_and_marshals_its_arguments():
    """Every ValueError of poseGraphWideBatch: poseGraphBatch's recorded message for the same fault (the limit cases have
    the new limits), the checks in the same order (first+last: a fault of the first and of the last argument together
    gives the first one's message), and nothing reaches the library.  The good calls pass poseGraphBatch's recorded
    arguments followed by the work output."""
    import json
    tw, base, good, refused = wrapper_spec()
    record = json.load(open(tw.RECORD))["wrappers"]["poseGraphBatch"]
    assert set(refused) == set(record["refused"]) and "first+last" in refused
    for case, change in refused.items():
        msg = run_wrapper(tw, base, change, True)
        if case in ("vertex-limit", "edge-limit"):
            assert msg == "at most 65536 vertices and 1048576 edges per graph", case
        else:
            assert msg == record["refused"][case], case
    assert record["refused"]["first+last"] == record["refused"]["sims-dtype"]
    for case, change in good.items():
        got = run_wrapper(tw, base, change, False)
        assert got["fn"] == "pislam_pose_graph_wide_batch", case
        B, V, E = (1, MAX_V + 1, MAX_E + 1) if case == "old-limits-passed" else (tw.B, tw.V, tw.E)
        assert [r["shape"] for r in got["returns"]] == [[B, V, 13], [B], [B], [B, 2]], case
        assert [r["dtype"] for r in got["returns"]] == ["float32", "float64", "int32", "int32"], case
        if case == "old-limits-passed":
            assert got["args"][11:14] == [V, E, B]
            continue
        old = record["good"][case]["calls"][0]["args"]
        given = case == "outputs-given"
        assert got["args"] == old + ["work" if given else "new:3"], case
        assert got["returns"][3]["given"] == ("work" if given else None)
        if case == "in-place":
            assert got["returns"][0]["given"] == "sims"
    # the reserve call: the three sizes, checked
    from pislam_amd import frontend as fe
    ctx = tw.Recorder()
    fe.reservePoseGraphWide(WIDE_MAX_V, WIDE_MAX_E, 3, ctx=ctx)
    assert [(n, a[1:]) for n, a in ctx.calls] == [("pislam_pose_graph_wide_reserve", (WIDE_MAX_V, WIDE_MAX_E, 3))]
    assert ctx.checked == ["pislam_pose_graph_wide_reserve"]


# ---- GPU tests --------------------------------------------------------------------------------------------------------
class WideDevice(Device):
    """tg.Device through the new call: a work output beside the others; within the old limits every run is repeated
    through pislam_pose_graph_batch on the same device buffers and must give the same bytes, sentinels included."""

    def sentinels(self, B, V):
        t = self.torch
        return dict(super().sentinels(B, V), work=t.full((B, 2), SENT, dtype=t.int32, device="cuda"))

    def call_old(self, prm, d, shape, B, o):
        return Device.call(self, prm, d, shape, B, o)

    def call(self, prm, d, shape, B, o):
        ptr = self.capi.ptr
        p = None if prm is None else self.capi.PoseGraphParams(*prm)
        return self.lib.pislam_pose_graph_wide_batch(
            self.ctx.h, None if p is None else ctypes.byref(p), ptr(d["sims"]), ptr(d["v_counts"]), ptr(d["fixed"]),
            ptr(d["edges"]), ptr(d["meas"]), ptr(d.get("weight")), ptr(d["e_counts"]), ptr(d["inc_ptr"]), ptr(d["inc"]),
            shape[0], shape[1], B, ptr(o["sims_out"]), ptr(o["cost"]), ptr(o["status"]), ptr(o.get("work")))

    def run_packed(self, h, prm, shape):
        B = len(h["v_counts"])
        d = self.upload(h)
        o = self.sentinels(B, shape[0])
        assert self.call(prm, d, shape, B, o) == 0, self.lib.pislam_last_error(self.ctx.h)
        self.ctx.synchronize()
        got = {k: v.cpu().numpy() for k, v in o.items()}
        if shape[0] <= MAX_V and shape[1] <= MAX_E:
            o2 = Device.sentinels(self, B, shape[0])
            assert self.call_old(prm, d, shape, B, o2) == 0, self.lib.pislam_last_error(self.ctx.h)
            self.ctx.synchronize()
            for k, v in o2.items():
                assert v.cpu().numpy().tobytes() == got[k].tobytes(), "%s differs from pislam_pose_graph_batch's" % k
        for k, v in h.items():                                 # no input was written
            assert v is None or d[k].cpu().numpy().tobytes() == v.tobytes(), k
        return got

    def run(self, graphs, prm, shape, counts=None, weighted=None):
        return self.run_packed(self.pack(graphs, *shape, counts=counts, weighted=weighted), prm, shape)


def assert_wide(got, want, graphs, what=""):
    """assert_graphs, and the work words: the device walked the probe's path."""
    assert_graphs(got, want, graphs, what)
    for b, x in enumerate(want):
        ran = x["status"] & 255 == 0
        assert got["work"][b].tolist() == ([x["solves"], x["cg"]] if ran else [0, 0]), (what, b, got["work"][b], x["solves"], x["cg"])
        assert ran or (x["solves"], x["cg"]) == (0, 0)


@pytest.mark.gpu
def test_wide_smallest_graph(gpu_ctx):
    g = two_vertices(11)
    want = probe([g], [DEFAULT])
    assert want[0]["status"] & 255 == 0 and bits(want[0]["sims"]) != bits(g["sims"])
    assert_wide(WideDevice(gpu_ctx).run([g], DEFAULT, (2, 1)), want, [g], "smallest")


@pytest.mark.gpu
def test_wide_every_case_in_batches_with_unequal_counts(gpu_ctx):
    """tg's test of the same name through the new call: one batch per parameter set, padded strides, graphs whose counts
    are 0, PISLAM_COUNT_INVALID and beyond the strides; with weights and with weight == NULL."""
    groups = {}
    for name, g, prm in cases():
        groups.setdefault(prm, []).append(g)
    for prm, gs in groups.items():
        for weighted in (True, False):
            use = gs if weighted else [g for g in gs if g.get("weight") is None]
            V, E = shape_of(use)
            full = make_graph(77, nv=V, extra=E - V, drift=3.0 / V, loops=((-1, 0),) if E >= V else ())
            assert shape_of([full]) == (V, E)
            batch = use + [EMPTY, EMPTY, full]
            counts = [None] * len(use) + [(0, 0), (COUNT_INVALID, COUNT_INVALID), (V + 3, E + 9)]
            pad = (3, 5) if weighted else (0, 0)
            got = WideDevice(gpu_ctx).run(batch, prm, (V + pad[0], E + pad[1]), counts if not any(pad) else counts[:-1] + [None],
                                          weighted=weighted)
            want = probe(batch, [prm] * len(batch))
            assert want[len(use)]["status"] == 3 and want[-1]["status"] & 255 == 0
            assert_wide(got, want, batch, "%r weighted %r" % (prm, weighted))


@functools.lru_cache(maxsize=None)
def group_boundary_graphs():
    """Beside tg.boundary_graphs() (255, 256, 257 and 1025 vertices, a vertex of degree 300): 255, 256 and 257 edges; free
    vertices at the multiples of 256 among 1024 only, which all fall into partial 0; 257 vertices and 257 edges, so that
    only the last vertex and the last edge lie in the second group of 256."""
    gs = [make_graph(60 + n, nv=n - 19, extra=19, drift=0.2) for n in (255, 256, 257)]
    assert [len(g["edges"]) for g in gs] == [255, 256, 257]
    fx = np.ones(1024, np.uint8)
    fx[::256] = 0
    gs.append(make_graph(64, nv=1024, extra=300, drift=0.05, fixed=np.flatnonzero(fx)))
    assert gs[-1]["fixed"].sum() == 1020 and not gs[-1]["fixed"][[0, 256, 512, 768]].any()
    last = make_graph(65, nv=257, extra=0, drift=0.2)
    assert shape_of([last]) == (257, 257) and 256 in last["edges"][256]
    return gs + [last]


@pytest.mark.gpu
def test_wide_group_and_partial_boundaries(gpu_ctx):
    gs = list(boundary_graphs()) + group_boundary_graphs()
    want = probe(gs, [BIG] * len(gs))
    assert all(x["status"] & 255 == 0 and x["status"] >> 8 >= 2 for x in want)
    assert_wide(WideDevice(gpu_ctx).run(gs, BIG, shape_of(gs)), want, gs, "boundaries")
    # a free vertex with no edge: every solve fails, and the state is kept
    base = make_graph(10, nv=6, extra=2)
    lone = graph(np.concatenate([base["sims"], base["sims"][:1]]), np.concatenate([base["fixed"], [0]]), base["edges"], base["meas"])
    want = probe([lone], [SMALL])
    assert want[0]["status"] == 1 << 8 and want[0]["solves"] == SMALL[0] and want[0]["cg"] == 0
    assert_wide(WideDevice(gpu_ctx).run([lone], SMALL, shape_of([lone])), want, [lone], "lone vertex")


def refused_graphs():
    """Every way tests/test_pose_graph.py provokes the codes 1, 2 and 3, by name."""
    out = [(name, g) for name, g, prm in cases() if name.startswith("code_")]
    assert {name[:6] for name, _ in out} == {"code_1", "code_2", "code_3"} and len(out) == 14
    for want in ("bad_index", "entry_on_the_wrong_side", "no_fixed_vertex", "nan", "scale_not_positive", "edge_rotated_by_pi",
                 "no_edge", "no_free_vertex"):
        assert any(want in name for name, _ in out), want
    return out


@pytest.mark.gpu
def test_wide_refused_graphs_between_accepted_ones(gpu_ctx):
    """Each refused graph with an accepted graph before and after it: it copies its inputs, its neighbours are those of a
    batch without it."""
    ok = [make_graph(80 + k, nv=7 + k % 3, extra=2) for k in range(3)]
    batch, names = [], []
    for k, (name, g) in enumerate(refused_graphs()):
        batch += [ok[k % 3], g]
        names += ["ok", name]
    batch.append(ok[0]), names.append("ok")
    want = probe(batch, [SMALL] * len(batch))
    for name, g, x in zip(names, batch, want):
        if name == "ok":
            assert x["status"] & 255 == 0 and bits(x["sims"]) != bits(g["sims"])
        else:
            assert x["status"] == int(name[5]) and x["cost"] == 0.0 and bits(x["sims"]) == bits(g["sims"]), name
    got = WideDevice(gpu_ctx).run(batch, SMALL, shape_of(batch, (1, 2)), weighted=True)
    assert_wide(got, want, batch, "refused between accepted")
    alone = WideDevice(gpu_ctx).run(ok, SMALL, shape_of(batch, (1, 2)), weighted=True)
    for k in range(3):
        for b in [i for i, g in enumerate(batch) if g is ok[k]]:
            for key in ("sims_out", "cost", "status", "work"):
                assert got[key][b].tobytes() == alone[key][k].tobytes(), (key, b)


@pytest.mark.gpu
def test_wide_more_graphs_than_any_grid(gpu_ctx):
    """65537 two-vertex graphs, one more (graph, group) pair than the grid cap: the last is walked in a second pass.  Every
    fifth is refused (codes 3 and 2 in turn); seven distinct seeds."""
    B, prm = 65537, (4, 8, 1e-6, 1e-9)
    kinds = [two_vertices(1000 + k) for k in range(7)]
    kinds.append(edit(kinds[0], fixed=np.zeros(2, np.uint8)))          # code 3
    s = kinds[1]["sims"].copy()
    s[1, 5] = np.nan
    kinds.append(edit(kinds[1], sims=s))                               # code 2
    want = probe(kinds, [prm] * len(kinds))
    assert [x["status"] & 255 for x in want] == [0] * 7 + [3, 2] and len({x["sims"].tobytes() for x in want}) == 9
    which = np.arange(B) % 7
    which[::5] = 7 + (np.arange(B)[::5] // 5) % 2
    assert which[B - 1] < 7 and which[65535] == 8
    d = WideDevice(gpu_ctx)
    small = d.pack(kinds, 2, 1)
    got = d.run_packed({k: (None if v is None else np.ascontiguousarray(v[which])) for k, v in small.items()}, prm, (2, 1))
    exp = dict(sims_out=np.stack([x["sims"] for x in want]).astype(F32), cost=np.array([x["cost"] for x in want]),
               status=np.array([x["status"] for x in want], np.uint32),
               work=np.array([[x["solves"], x["cg"]] if x["status"] & 255 == 0 else [0, 0] for x in want], np.uint32))
    for key, v in exp.items():
        assert v.dtype.itemsize == got[key].dtype.itemsize and got[key].tobytes() == np.ascontiguousarray(v[which]).tobytes(), key


@pytest.mark.gpu
def test_wide_just_past_the_old_limits(gpu_ctx):
    g, want = past_the_old_limits(), past_the_old_limits_want()
    assert want["status"] == 3 << 8 and want["cg"] == 16
    assert_wide(WideDevice(gpu_ctx).run([g], PAST_PRM, shape_of([g])), [want], [g], "4097 vertices, 16385 edges")


@pytest.mark.gpu
def test_wide_at_the_new_limits(gpu_ctx):
    """One graph of 65536 vertices and 2^20 edges (a ring and the chords of strides 2 to 16), one Levenberg iteration of two
    conjugate-gradient iterations, against the probe through the binary case file."""
    g = ring_with_chords(WIDE_MAX_V, WIDE_MAX_E, 5)
    assert shape_of([g]) == (WIDE_MAX_V, WIDE_MAX_E) and int(g["inc"].max()) == 2 * WIDE_MAX_E - 1
    prm = (1, 2, 1e-6, 1e-9)
    want = wide_probe([g], [prm])
    assert want[0]["status"] == 2 << 8 and (want[0]["solves"], want[0]["cg"]) == (1, 2) and bits(want[0]["sims"]) != bits(g["sims"])
    assert_wide(WideDevice(gpu_ctx).run([g], prm, (WIDE_MAX_V, WIDE_MAX_E)), want, [g], "the new limits")


@pytest.mark.gpu
def test_wide_seeded_family_equals_the_probe(gpu_ctx):
    """The 256 seeds of test_backend_fuzz's pose_graph row (all six parameter sets, every edit, workgroup-sized graphs
    included) through the new call; the expectation is the row's own."""
    fam = tf.family("pose_graph")
    seen = [c for _, cs, _ in fam for c in cs]
    assert len(seen) >= 64 and {c["edit"] for c in seen} == set(tf.GRAPH_EDITS) and {c["big"] for c in seen} == {False, True}
    assert [s for s, _, _ in fam] == list(range(len(tf.GRAPH_SETS))) == list(range(6))
    d = WideDevice(gpu_ctx)
    for s, cs, want in fam:
        prm, weighted = tf.GRAPH_SETS[s]
        items = [c["item"] for c in cs]
        got = d.run(items, prm, shape_of(items, (1, 2)), weighted=weighted)
        assert_wide(got, want, items, "parameter set %d" % s)


@pytest.mark.gpu
def test_wide_in_place_and_refusals(gpu_ctx):
    d = WideDevice(gpu_ctx)
    gs = [make_graph(41, nv=9, extra=4, weights=True), make_graph(42, nv=5, extra=1, weights=True)]
    V, E = shape = shape_of(gs, (2, 3))
    B = len(gs)
    h = d.pack(gs, *shape)
    dev = d.upload(h)
    o = d.sentinels(B, V)
    good = DEFAULT
    reserve = d.lib.pislam_pose_graph_wide_reserve
    for prm in ((0, 256, 1e-6, 1e-9), (65, 256, 1e-6, 1e-9), (20, 0, 1e-6, 1e-9), (20, 1025, 1e-6, 1e-9), (20, 256, -1e-6, 1e-9),
                (20, 256, 1.0, 1e-9), (20, 256, float("nan"), 1e-9), (20, 256, 1e-6, -1e-9), (20, 256, 1e-6, float("nan")), None):
        assert d.call(prm, dev, shape, B, o) == -1, prm
    for bad in ((0, E), (WIDE_MAX_V + 1, E), (V, 0), (V, WIDE_MAX_E + 1)):
        assert d.call(good, dev, bad, B, o) == -1, bad
        assert reserve(gpu_ctx.h, bad[0], bad[1], B) == -1, bad
    assert d.call(good, dev, shape, -1, o) == -1 and reserve(gpu_ctx.h, V, E, -1) == -1
    host = np.zeros(B * (V + 1) * 13 + B * E * 13, np.int32)
    for name in ("sims", "v_counts", "fixed", "edges", "meas", "weight", "e_counts", "inc_ptr", "inc", "sims_out", "cost", "status",
                 "work"):
        for repl in (None, host):                             # NULL, then a host pointer
            if name in ("weight", "work") and repl is None:
                continue
            ins, outs = dict(dev), dict(o)
            (ins if name in ins else outs)[name] = repl
            assert d.call(good, ins, shape, B, outs) == -1, name
    # overlaps: an output on an input, two outputs on each other (partly, too)
    assert d.call(good, dev, shape, B, dict(o, status=dev["v_counts"])) == -1
    assert d.call(good, dev, shape, B, dict(o, work=dev["inc"])) == -1
    assert d.call(good, dev, shape, B, dict(o, sims_out=dev["meas"])) == -1
    assert d.call(good, dev, shape, B, dict(o, sims_out=dev["sims"].view(-1)[13:])) == -1
    assert d.call(good, dev, shape, B, dict(o, cost=o["sims_out"].view(-1).view(d.torch.float64))) == -1
    assert d.call(good, dev, shape, B, dict(o, work=o["status"])) == -1
    gpu_ctx.synchronize()
    for k, v in o.items():
        assert (v.cpu().numpy().view(np.uint8) == 0x5A).all(), k
    assert dev["sims"].cpu().numpy().tobytes() == h["sims"].tobytes()
    # batch 0 is a no-op after the checks: the pointers are not looked at
    p = d.capi.PoseGraphParams(*good)
    assert d.lib.pislam_pose_graph_wide_batch(gpu_ctx.h, ctypes.byref(p), *([None] * 9), V, E, 0, None, None, None, None) == 0
    assert reserve(gpu_ctx.h, V, E, 0) == 0
    # work == NULL: the other outputs are the same
    want = probe(gs, [good] * B)
    assert all(x["status"] & 255 == 0 for x in want)
    none = d.sentinels(B, V)
    assert d.call(good, dev, shape, B, dict(none, work=None)) == 0
    gpu_ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in none.items()}
    assert_graphs(got, want, gs, "work == NULL")
    assert (got["work"].view(np.uint32) == SENT).all()
    # sims_out may be sims; nothing is written at or beyond the counts
    assert d.call(good, dev, shape, B, dict(o, sims_out=dev["sims"])) == 0
    gpu_ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["sims_out"] = dev["sims"].cpu().numpy()
    for b, g in enumerate(gs):                                # beyond the counts the inputs' rubbish is untouched
        nv = len(g["sims"])
        assert got["sims_out"][b, nv:].tobytes() == h["sims"][b, nv:].tobytes()
        got["sims_out"][b, nv:].view(np.uint32)[...] = SENT
    assert_wide(got, want, gs, "in place")


@pytest.mark.gpu
def test_wide_determinism_and_graph_replay(gpu_ctx):
    """Two calls give the same bits; after reservePoseGraphWide on a fresh context the call is captured on a side stream
    without a warm-up call, and both replays write what the eager call wrote."""
    import torch as t
    from pislam_amd.capi import Context
    from pislam_amd.frontend import poseGraphWideBatch, reservePoseGraphWide
    d = WideDevice(gpu_ctx)
    gs = [make_graph(51, nv=20, extra=10), make_graph(52, nv=7, extra=2), edit(make_graph(53, nv=5), fixed=np.zeros(5, np.uint8))]
    shape = shape_of(gs)
    dev = d.upload(d.pack(gs, *shape))
    args = (dev["sims"], dev["v_counts"], dev["fixed"], dev["edges"], dev["meas"], dev["weight"], dev["e_counts"], dev["inc_ptr"],
            dev["inc"])
    kw = dict(zip(PG_FIELDS, (6, 24, 1e-6, 1e-9)))
    first = [x.cpu().numpy().copy() for x in poseGraphWideBatch(*args, ctx=gpu_ctx, **kw, **d.sentinels(3, shape[0]))]
    again = [x.cpu().numpy().copy() for x in poseGraphWideBatch(*args, ctx=gpu_ctx, **kw, **d.sentinels(3, shape[0]))]
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    want = probe(gs, [tuple(kw.values())] * 3)
    assert [x["status"] & 255 for x in want] == [0, 0, 3]
    assert_wide(dict(zip(("sims_out", "cost", "status", "work"), first)), want, gs, "frontend")
    gpu_ctx.synchronize()
    t.cuda.synchronize()
    side = t.cuda.Stream(t.device("cuda:0"))
    with t.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        reservePoseGraphWide(*shape, 3, ctx=ctx)
        o = d.sentinels(3, shape[0])
        side.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=side):
            poseGraphWideBatch(*args, ctx=ctx, **kw, **o)
        for _ in range(2):
            for x in o.values():
                x.view(t.uint8).fill_(0x5A)
            g.replay()
            side.synchronize()
            for a, b in zip(first, o.values()):
                assert a.tobytes() == b.cpu().numpy().tobytes()
        ctx.close()


@pytest.mark.gpu
def test_wide_chain_from_the_covisibility_graph_of_a_large_map(gpu_ctx):
    """The chain that stops at essentialGraph without `wide`: 2100 key frames, each sharing two points with each of its
    eight successors, give covisibilityBatch -> essentialPairs 16764 edges; with the loop edge the graph has 16765, more
    than pislam_pose_graph_batch takes.  essentialGraph(wide=True) -> poseGraphWideBatch -> correctMapPointsBatch: the
    graph is accepted, its cost falls, and the similarities and the moved points are the probe's."""
    import torch
    from pislam_amd.frontend import (correctMapPointsBatch, covisibilityBatch, essentialGraph, essentialPairs, mapObservations,
                                     poseGraphWideBatch, relativeSim3)
    K, D, SHARED = 2100, 8, 2
    i, dd = np.meshgrid(np.arange(K), np.arange(1, D + 1), indexing="ij")
    keep = i + dd < K
    a, b = i[keep], (i + dd)[keep]
    links = len(a)
    assert links == D * K - D * (D + 1) // 2 == 16764 > MAX_E
    pt = np.repeat(np.arange(links * SHARED), 2).astype(np.int32)
    kf = np.stack([np.repeat(a, SHARED), np.repeat(b, SHARED)], 1).reshape(-1).astype(np.int16)
    rng = np.random.default_rng(3)
    shuffle = rng.permutation(len(pt))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    okf, opt, counts = mapObservations(up(kf[shuffle][None]), up(pt[shuffle][None]), up(np.array([len(pt)], np.int32)))
    nk = up(np.array([K], np.int32))
    outs = covisibilityBatch(okf, opt, counts, nk, kf_stride=K, min_weight=SHARED, ctx=gpu_ctx)
    gpu_ctx.synchronize()
    assert int(outs[6][0]) == 0
    pairs = essentialPairs(*outs[:4], nk, min_weight=SHARED)[0]
    assert len(pairs) == links
    sims = np.zeros((K, 13), F32)
    sims[:, [0, 4, 8, 12]] = 1.0
    sims[:, 9] = 0.3 * np.arange(K) + rng.normal(0, 0.01, K)
    d_sims = up(sims)
    loop = relativeSim3(d_sims[0:1], d_sims[K - 1:K])
    loop[0, 9] += 0.05                                       # the loop edge disagrees with the drifted chain
    with_loop = torch.cat([pairs, torch.tensor([[0, K - 1]], dtype=torch.int32, device="cuda")])
    fixed = torch.zeros(K, dtype=torch.uint8, device="cuda")
    fixed[0] = 1
    with pytest.raises(ValueError):
        essentialGraph(d_sims, fixed, with_loop, meas=loop)
    G = essentialGraph(d_sims, fixed, with_loop, meas=loop, wide=True)
    assert tuple(G[3].shape) == (1, links + 1, 2)
    prm = (3, 64, 1e-6, 1e-9)
    sims_new, cost, status, work = poseGraphWideBatch(*G, **dict(zip(PG_FIELDS, prm)), ctx=gpu_ctx)
    gpu_ctx.synchronize()
    word = lambda x: x[0].cpu().numpy().view(np.uint32)
    g = dict(sims=G[0][0].cpu().numpy(), fixed=G[2][0].cpu().numpy(), edges=word(G[3]), meas=G[4][0].cpu().numpy(), weight=None,
             inc_ptr=word(G[7]), inc=word(G[8]))
    want = wide_probe([g], [prm])[0]
    F0 = float(tg.RefGraph(g).evaluate(g["sims"].astype(F64))[1])
    got = dict(sims_out=sims_new.cpu().numpy(), cost=cost.cpu().numpy(), status=status.cpu().numpy().view(np.uint32),
               work=work.cpu().numpy().view(np.uint32))
    tg.assert_same(dict(status=int(got["status"][0]), cost=float(got["cost"][0]), sims=got["sims_out"][0]), want, "chain")
    assert got["work"][0].tolist() == [want["solves"], want["cg"]]
    assert want["status"] & 255 == 0 and want["status"] >> 8 >= 2
    print("cost %.3g from %.3g" % (want["cost"], F0))
    assert 0.05 ** 2 * 0.99 < F0 and want["cost"] < F0
    npt = 200
    ref = rng.integers(0, K, npt).astype(np.int16)
    xw = rng.uniform(-6, 6, (npt, 3)).astype(F32)
    xw2, st = correctMapPointsBatch(up(xw[None]), up(ref[None]), up(np.array([npt], np.int32)), G[0], sims_new, G[1], ctx=gpu_ctx)
    gpu_ctx.synchronize()
    pts, pst = tg.probe_points(sims, want["sims"], ref, xw)
    assert int(st.sum()) == 0 == int(pst.sum()) and bits(xw2[0].cpu().numpy()) == bits(pts)
    assert (pts != xw).any()
