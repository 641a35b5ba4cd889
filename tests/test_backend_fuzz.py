"""Seeded fuzzing of the back-end kernels against their host probes.

Every back-end kernel has a numpy restatement of its contract, a host probe (its own *_math.h under the host compiler)
and GPU tests that compare the library with one of the two word for word, in a module of its own.  What reaches the GPU
there is a few dozen hand-built cases of one scene family.  Here a generator draws hundreds of cases per kernel whose
numbers provoke the data-dependent control flow (rejected Levenberg steps, failed factorisations, points crossing Z_MIN,
chi2 at its bound, tied RANSAC scores, conjugate-gradient runs that stop early), and the GPU is compared with the probe.

Nothing is restated here.  ROWS has one row per kernel: the module whose scene builders, probe_line / case_line,
restatement, Device and assert_* it uses, the probe's name, the parameter sets, the hostile edits and how results compare.

case(kernel, seed) is deterministic in (kernel, seed) and draws
  1. a shape: three quarters small (at most 64 observations, matches or edges), the rest at a boundary of the kernel's
     decomposition +- 1 (the constants are read out of the kernels' headers),
  2. one of the row's parameter sets (parameters are per call: the cases that share a set make one batch),
  3. one hostile edit: the row's edits in turn by seed, so that any len(edits) consecutive seeds hold every kind.  The
     refusal kinds (non-finite inputs, malformed index lists) are one entry of at least ten.

CPU tests, per kernel: the probe equals the module's restatement on every output word of the first SAMPLE cases, and the
family of the GPU test meets conditions that the probe's outputs alone show (every status code, the share of normal ends,
early stops, distinct outputs); for the RANSAC kernels the share of tied best scores comes from the restated hypotheses
of the sample, since the probe prints the winner only.  GPU tests, per kernel: FAMILY cases, one call per parameter set
through the module's Device, every output word and sentinel against the probe.  tests/backend_fuzz_campaign.py runs the
same generator and comparison over any number of seeds.

The measured shares stand next to their floors (half of the measured value)."""
import functools
import os
import re
import shutil
import subprocess
import tempfile
import time
import types

import numpy as np
import pytest

import test_covisibility as tcov
import test_local_ba as tba
import test_pnp_ransac as tpnp
import test_pose_graph as tg
import test_pose_refine as tpose
import test_sim3_ransac as tsim
import test_sim3_refine as tref
import test_triangulate as ttri
import test_two_view as ttv
import test_two_view_reconstruct as trec
from conftest import ROOT

F32, F64 = np.float32, np.float64
MONO = tpose.MONO
FIRST_SEED = 40000                               # the tests' family: seeds FIRST_SEED .. FIRST_SEED + FAMILY - 1
FAMILY = 256
SAMPLE = 48                                      # the restated cases: at least 24, and every edit kind


# ---- the decomposition constants, out of the headers --------------------------------------------------------------------
def constant(header, name):
    text = open(os.path.join(ROOT, "pislam_amd", "csrc", header)).read()
    return int(re.search(r"constexpr int %s = (\d+)[;,]" % name, text).group(1))


WG = constant("pislam_refine_kernels.h", "THREADS")               # the refinement, BA and graph kernels' workgroup
WG_RANSAC = constant("pislam_ransac_kernels.h", "THREADS")       # the three RANSAC kernels' workgroup
WG_RECON = constant("pislam_recon_kernels.h", "RC_THREADS")
WG_TRI = constant("pislam_mappoint_kernels.h", "MP_THREADS")
WG_COVIS = constant("pislam_covis_kernels.h", "CV_THREADS")
POSE_RESIDENT = constant("pislam_pose_kernels.h", "PO_RES") * WG
REFINE_RESIDENT = constant("pislam_sim3_refine_kernels.h", "SR_RES") * WG
BA_MAX_KF, BA_MAX_FREE = (int(v) for v in re.search(
    r"constexpr int MAX_KF = (\d+), MAX_FREE = (\d+)", open(os.path.join(ROOT, "pislam_amd", "csrc", "pislam_ba_math.h")).read()).groups())
HYPOTHESES = (1, 63, 64, 65, constant("pislam_ransac_math.h", "MAX_HYP"))


def around(rng, *boundaries):
    return int(rng.choice(boundaries)) + int(rng.integers(-1, 2))


# ---- the probes -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probe_exe(name):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(tempfile.mkdtemp(prefix=name + "_"), name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", name + ".cpp"), "-o", exe])
    return exe


def run_probe(name, lines):
    """The output lines of tools/probes/<name>.cpp, one per case line."""
    if not lines:
        return []
    exe = probe_exe(name)
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        got = subprocess.run([exe, f.name], check=True, capture_output=True, text=True).stdout.splitlines()
    finally:
        os.unlink(f.name)
    assert len(got) == len(lines), (name, len(got), len(lines))
    return got


def words(tokens):
    return np.array([int(x, 16) for x in tokens], np.uint32).view(F32)


def f64_of(token):
    return float(np.array([int(token, 16)], np.uint64).view(F64)[0])


def bits_of(token):
    return np.zeros(0, np.uint8) if token == "-" else np.array([int(c) for c in token], np.uint8)


def same_by_line(result_line):
    def same(got, want, tag):
        assert result_line(got) == result_line(want), tag
    return same


def pixels(u):
    with np.errstate(all="ignore"):
        return np.clip(np.rint(np.nan_to_num(np.asarray(u, F64) * 256, nan=0.0, posinf=2.0 ** 30, neginf=-2.0 ** 30)),
                       -2.0 ** 30, 2.0 ** 30).astype(np.int64)


Q8_EXTREMES = np.array([[1 << 22, -(1 << 22), (1 << 22) - 1], [(1 << 22) + 1, -(1 << 22) - 1, 1 << 22],
                        [1 << 30, -(1 << 30), (1 << 31) - 1], [-(1 << 31) + 1, (1 << 31) - 1, MONO]], np.int64)


def some(rng, n, k):
    return rng.choice(n, min(n, k), replace=False) if n else np.zeros(0, np.int64)


def twice(a, n):
    """Every entry of a twice, n entries in all."""
    h = (n + 1) // 2
    return np.concatenate([a[:h], a[:n - h]])


# ==== pislam_pose_refine_batch ==============================================================================================
POSE_TAB = np.concatenate([tpose.ref_level_weights(8), [tpose.TH_MONO / F32(4), np.nextafter(tpose.TH_MONO, F32(9)) / F32(4),
                                                        tpose.TH_STEREO / F32(4), np.nextafter(tpose.TH_STEREO, F32(9)) / F32(4)]]).astype(F32)
# rounds, iters, huber_rounds, min_obs, eps, with levels: one round; the most rounds and iterations with every round
# robust and eps 0; no robust round; a min_obs above every small count
POSE_SETS = [(4, 10, 3, 10, 1e-6, True), (1, 1, 0, 3, 0.0, True), (8, 32, 8, 3, 0.0, True), (4, 10, 0, 10, 0.0, False),
             (2, 3, 2, 10, 1e-3, True), (3, 6, 1, 200, 1e-6, False)]
POSE_EDITS = ["none", "depth", "far", "plane", "line", "focal_small", "focal_large", "far_start", "outliers", "chi2_at_th",
              "q8", "level", "duplicate", "singular", "refused"]
Z_DEPTHS = np.array([[0, 0, 0], [0, 0, tpose.Z_MIN], [0, 0, np.nextafter(tpose.Z_MIN, F32(0))], [0, 0, -1],
                     [1e-4, 0, np.nextafter(tpose.Z_MIN, F32(1))]], F32)


def observe(xw, truth, cam, obs):
    """The Q8 observations of xw under the pose truth = (R, t) and the camera, stereo where obs is."""
    R, t = truth
    fx, fy, cx, cy, bf = (float(c) for c in cam)
    xc = np.asarray(xw, F64) @ R.T + t
    with np.errstate(all="ignore"):
        u, v = fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy
        out = np.stack([pixels(u), pixels(v), pixels(u - bf / xc[:, 2])], 1)
    out[:, 2] = np.where(obs[:, 2] == MONO, MONO, out[:, 2])
    return out


def on_a_line(rng, n, centre=(0, 0, 8)):
    d = rng.normal(0, 1, 3)
    return (np.asarray(centre, F64) + rng.uniform(-3, 3, n)[:, None] * d / np.linalg.norm(d)).astype(F32)


def pose_make(rng, seed, st, edit, big):
    n = around(rng, WG, POSE_RESIDENT) if big else int(rng.integers(1, 65))
    kw = dict(n=n, stereo=float(rng.choice([0.0, 0.5, 1.0])), outliers=float(rng.choice([0.0, 0.1, 0.3])))
    if edit == "far_start":
        kw.update(rot=0.5, trans=2.0)
    if edit == "outliers":
        kw.update(outliers=0.5)
    fr, truth, _ = tpose.scene(int(rng.integers(1 << 31)), **kw)
    fr["tab"] = POSE_TAB
    if edit == "depth":                                      # at the first pose, the identity
        idx = some(rng, n, 5)
        fr["xw"][idx] = Z_DEPTHS[:len(idx)]
    elif edit == "far":                                      # the scene some km away, the start moved with it
        off = rng.choice([-1.0, 1.0], 3) * rng.uniform(2000, 6000, 3)
        fr["xw"] = (fr["xw"].astype(F64) + off).astype(F32)
        fr["pose"][9:] = (-off).astype(F32)
    elif edit == "plane":
        fr["xw"][:, 2] = 6
        fr["obs"] = observe(fr["xw"], truth, fr["cam"], fr["obs"])
    elif edit == "line":
        fr["xw"] = on_a_line(rng, n)
        fr["obs"] = observe(fr["xw"], truth, fr["cam"], fr["obs"])
    elif edit in ("focal_small", "focal_large"):
        fr["cam"][:2] *= F32(0.01 if edit == "focal_small" else 50)
    elif edit == "chi2_at_th":                               # e = 2 px and w = th / 4: chi2 is th and one ulp above
        for i, (lv, stereo) in enumerate(((8, 0), (9, 0), (10, 1), (11, 1))[:n]):
            fr["xw"][i], fr["level"][i] = (0, 0, 1), lv
            fr["obs"][i] = (322 * 256, 240 * 256, 270 * 256 if stereo else MONO)
    elif edit == "q8":
        idx = some(rng, n, 4)
        fr["obs"][idx] = Q8_EXTREMES[:len(idx)]
    elif edit == "level":                                    # at and above nlevels
        idx = some(rng, n, 3)
        fr["level"][idx] = np.array([len(POSE_TAB), len(POSE_TAB) + 1, 255], np.uint8)[:len(idx)]
    elif edit == "duplicate":
        for k in ("xw", "obs", "level"):
            fr[k] = twice(fr[k], n)
    elif edit == "singular":                                 # every point the same: no 6 x 6 factor
        fr["xw"][:], fr["obs"][:], fr["level"][:] = fr["xw"][0], fr["obs"][0], 0
        fr["obs"][:, 2] = fr["obs"][0, 0] - 2000
    elif edit == "refused":
        kind = int(rng.integers(3))
        if kind == 0:
            fr["pose"][int(rng.integers(12))] = np.nan
        elif kind == 1:
            fr["cam"][int(rng.integers(5))] = np.inf
        else:
            fr["xw"][some(rng, n, 2)] = np.nan               # not refused: the observation is dead
    return fr


def pose_item(fr, st):
    return fr if st[5] else dict(fr, level=None, tab=None)


def pose_parse(line):
    t = line.split()
    return dict(status=int(t[0]), ninliers=int(t[1]), cost=f64_of(t[2]), pose=words(t[3:15]), inlier=bits_of(t[15]))


def pose_launch(ctx, st, items):
    ns = [len(fr["obs"]) for fr in items]
    return tpose.Device(ctx).run(items, ns, max(ns) + 1, st[:5], st[5])


def levenberg_row(**kw):
    return types.SimpleNamespace(codes={0, 1, 2}, code=lambda w: w["status"] & 255, ran=lambda w: w["status"] & 255 == 0,
                                 twins=("refused", "singular"), tied=None, sample=None, **kw)


POSE = levenberg_row(
    module=tpose, probe="pose_host_check", sets=POSE_SETS, edits=POSE_EDITS, needs={}, make=pose_make,
    lines=lambda st, items: [tpose.probe_line(pose_item(fr, st), st[:5]) for fr in items],
    parse=lambda st, items, got: [pose_parse(g) for g in got],
    restate=lambda st, items, b: tpose.ref_frame(pose_item(items[b], st), st[:5]),
    same=same_by_line(tpose.result_line), launch=pose_launch,
    check=lambda got, want, items: tpose.assert_frames(got, want, [len(fr["obs"]) for fr in items]),
    early=lambda st, w: w["status"] >> 8 < 1 + st[0] * (st[1] + 1), key=lambda w: w["pose"].tobytes() + np.array(w["cost"]).tobytes())


# ==== pislam_sim3_refine_batch ==============================================================================================
# rounds, iters, huber_rounds, min_obs, th2, fixed_scale, eps, with levels
REFINE_SETS = [(2, 5, 2, 10, 10.0, 0, 1e-6, True), (2, 5, 2, 10, 10.0, 1, 1e-6, False), (1, 1, 0, 3, 10.0, 0, 0.0, True),
               (8, 32, 8, 3, 6.0, 0, 0.0, True), (3, 8, 0, 200, 10.0, 1, 1e-6, True), (4, 10, 4, 10, 10.0, 0, 1e-3, False)]
REFINE_EDITS = ["none", "depth", "coincident", "plane", "line", "focal_small", "focal_large", "far_start", "outliers", "q8",
                "level", "duplicate", "masked", "singular", "tiny_scale", "refused"]
PAIR_KEYS = ("x1", "x2", "obs1", "obs2", "level1", "level2")


def sim3_observe(pr, truth, X2):
    """The pair with the camera-2 points X2, camera-1 points s R X2 + t and both sides' exact projections."""
    R, t, s = truth
    X1 = s * (np.asarray(X2, F64) @ R.T) + t
    q = lambda X, cam: np.concatenate([pixels(tsim.project(X, cam)), np.full((len(X), 1), MONO)], 1)
    with np.errstate(all="ignore"):
        return dict(pr, x1=X1.astype(F32), x2=np.asarray(X2, F32), obs1=q(X1, pr["cam1"]), obs2=q(np.asarray(X2, F64), pr["cam2"]))


def pair_edit(rng, pr, truth, edit, n):
    """The hostile edits that the Sim(3) RANSAC and the Sim(3) refinement share."""
    if edit == "depth":
        idx = some(rng, n, 5)
        pr["x2"][idx] = Z_DEPTHS[:len(idx)]
        idx = some(rng, n, 3)
        pr["x1"][idx] = Z_DEPTHS[:len(idx)]
    elif edit == "coincident":                               # both cameras at one place: the truth is the identity
        pr["x2"], pr["obs2"], pr["cam2"] = pr["x1"].copy(), pr["obs1"].copy(), pr["cam1"].copy()
    elif edit == "plane":
        X2 = pr["x2"].astype(F64)
        X2[:, 2] = 6
        pr = sim3_observe(pr, truth, X2)
    elif edit == "line":
        pr = sim3_observe(pr, truth, on_a_line(rng, n))
    elif edit in ("focal_small", "focal_large"):
        pr["cam1"][:2] *= F32(0.01 if edit == "focal_small" else 50)
    elif edit == "q8":
        idx = some(rng, n, 4)
        pr["obs1"][idx] = Q8_EXTREMES[:len(idx)]
        idx = some(rng, n, 2)
        pr["obs2"][idx] = Q8_EXTREMES[2:2 + len(idx)]
    elif edit == "level":
        idx = some(rng, n, 3)
        pr["level1"][idx] = np.array([len(tsim.TAB), len(tsim.TAB) + 1, 255], np.uint8)[:len(idx)]
        idx = some(rng, n, 2)
        pr["level2"][idx] = np.array([255, len(tsim.TAB)], np.uint8)[:len(idx)]
    elif edit == "duplicate":
        for k in PAIR_KEYS:
            pr[k] = twice(pr[k], n)
    return pr


def refine_make(rng, seed, st, edit, big):
    n = around(rng, WG, REFINE_RESIDENT) if big else int(rng.integers(1, 65))
    kw = dict(n=n, outliers=0.5 if edit == "outliers" else float(rng.choice([0.0, 0.1, 0.3])), fixed_scale=bool(st[5]))
    pr, truth, _ = tsim.scene(int(rng.integers(1 << 31)), levels=True, **kw)
    start = (0.2, 0.5, 0.3) if edit == "far_start" else (0.01, 0.05, 0.02)
    sim = tref.truth_sim(truth, start[0], start[1], 0.0 if st[5] else start[2], seed=int(rng.integers(1 << 31)))
    mask = tref.with_mask(n, int(rng.integers(1 << 31))) if rng.random() < 0.3 else None
    pr = pair_edit(rng, pr, truth, edit, n)
    if edit == "coincident":
        sim = tref.IDENTITY.copy()
    elif edit == "masked":
        mask = np.zeros(n, np.uint8)
    elif edit == "singular":                                 # the module's singular pin: H_22 is 0.0 exactly
        pr["x1"][:], pr["x2"][:], pr["level1"][:], pr["level2"][:] = (0, 0, 6), (0, 0, 4), 0, 1
        pr["obs1"][:, :2], pr["obs2"][:, :2] = (321 * 256, 240 * 256), (320 * 256, 241 * 256)
        sim = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 2, 1], F32)
    elif edit == "tiny_scale":
        sim[12] = F32(2.0 ** -20)
    elif edit == "refused":
        kind = int(rng.integers(4))
        if kind == 0:
            sim[int(rng.integers(13))] = np.nan
        elif kind == 1:
            sim[12] = F32(rng.choice([0.0, -1.0]))
        elif kind == 2:
            pr["cam%d" % (1 + int(rng.integers(2)))][int(rng.integers(5))] = np.nan
        else:
            pr["cam2"][int(rng.integers(2))] = 0
    return pr, sim, mask


def refine_item(it, st):
    return (it[0] if st[7] else tsim.no_levels(it[0])), it[1], it[2]


def refine_launch(ctx, st, items):
    ns = [len(it[0]["obs1"]) for it in items]
    return tref.Device(ctx).run([refine_item(it, st) for it in items], ns, max(ns) + 1, st[:7], st[7])


REFINE = levenberg_row(
    module=tref, probe="sim3_refine_host_check", sets=REFINE_SETS, edits=REFINE_EDITS, needs={}, make=refine_make,
    lines=lambda st, items: [tref.probe_line(*refine_item(it, st)[:2], st[:7], it[2]) for it in items],
    parse=lambda st, items, got: [tref.parse_result(g, len(it[0]["obs1"])) for g, it in zip(got, items)],
    restate=lambda st, items, b: tref.ref_refine(*refine_item(items[b], st)[:2], st[:7], items[b][2]),
    same=same_by_line(tref.result_line), launch=refine_launch,
    check=lambda got, want, items: tref.assert_pairs(got, want, [len(it[0]["obs1"]) for it in items]),
    early=lambda st, w: w["status"] >> 8 < 1 + st[0] * (st[1] + 1), key=lambda w: w["sim"].tobytes() + np.array(w["cost"]).tobytes())
REFINE.twins = ("refused", "singular", "masked")


# ==== pislam_local_ba_batch ===================================================================================================
# rounds, iters, huber_rounds, min_obs, eps, with levels
BA_SETS = [((2, (5, 10), 1, 10, 1e-6), True), ((1, (4,), 0, 4, 0.0), True), ((4, (32, 2, 32, 3), 4, 1, 0.0), True),
           ((2, (3, 4), 2, 4, 1e-2), False), ((3, (2, 4, 3), 0, 300, 1e-6), False), ((2, (6, 6), 1, 4, 1e-6), True)]
BA_EDITS = ["none", "depth", "far", "coincident", "plane", "focal_small", "focal_large", "far_start", "outliers", "level", "q8",
            "free_unobserved", "points_only", "refused"]
BA_PER_OBS = ("kf", "pt", "obs", "level")


def ba_cut(w, keep):
    for k in BA_PER_OBS:
        if k in w:
            w[k] = w[k][keep]
    return w


def ba_make(rng, seed, st, edit, big):
    kw = dict(noise=float(rng.choice([0, 0.5, 3])), gross=0.5 if edit == "outliers" else float(rng.choice([0, 0.05])),
              stereo=float(rng.choice([0, 0.5, 1])), start=100.0 if edit == "far_start" else float(rng.choice([0, 1, 10])))
    if big:                                                  # the workgroup size in observations, kf_free 15 and 16 of 32
        nkf, nfree, npt, n = BA_MAX_KF, BA_MAX_FREE - int(rng.integers(2)), 70, around(rng, WG)
        w = tba.make_window(int(rng.integers(1 << 31)), nkf=nkf, nfree=nfree, npt=npt, seen=0.3, min_seen=2, **kw)
    else:
        nkf = int(rng.integers(1, 9))
        nfree, npt, n = int(rng.integers(0, nkf + 1)), int(rng.integers(1, 30)), int(rng.integers(1, 65))
        w = tba.make_window(int(rng.integers(1 << 31)), nkf=nkf, nfree=nfree, npt=npt, seen=float(rng.uniform(0.3, 1)), **kw)
    w = ba_cut(w, slice(0, n))
    n = len(w["kf"])
    if edit == "depth":
        idx = some(rng, npt, 4)
        w["xw"][idx, 2] = np.array([0, tpose.Z_MIN, 1e-3, -1], F32)[:len(idx)]
    elif edit == "far":
        off = rng.choice([-1.0, 1.0], 3) * rng.uniform(2000, 6000, 3)
        w["xw"] = (w["xw"].astype(F64) + off).astype(F32)
        for k in range(nkf):
            R = w["poses"][k, :9].reshape(3, 3).astype(F64)
            w["poses"][k, 9:] = (w["poses"][k, 9:].astype(F64) - R @ off).astype(F32)
    elif edit == "coincident":
        w["poses"][:] = w["poses"][0]
    elif edit == "plane":
        w["xw"][:, 2] = 6
    elif edit in ("focal_small", "focal_large"):
        w["cams"][:, 0] *= F32(0.01 if edit == "focal_small" else 50)
    elif edit == "level":
        idx = some(rng, n, 3)
        w["level"][idx] = np.array([len(tba.TAB), len(tba.TAB) + 1, 255], np.uint8)[:len(idx)]
    elif edit == "q8":
        idx = some(rng, n, 4)
        w["obs"][idx] = Q8_EXTREMES[:len(idx)].astype(np.int32)
    elif edit == "free_unobserved":                          # a free key frame without an observation: no solve succeeds
        w["nfree"] = max(w["nfree"], 1)
        w = ba_cut(w, w["kf"] != 0)
    elif edit == "points_only":
        w["nfree"] = 0
    elif edit == "refused":
        kind = int(rng.integers(5))
        if kind == 0:
            w["xw"][int(rng.integers(npt)), int(rng.integers(3))] = np.inf
        elif kind == 1:
            w["cams"][int(rng.integers(nkf)), int(rng.integers(5))] = np.nan
        elif kind == 2 and n >= 2:
            w["pt"][0] = w["pt"][n - 1] + 1                  # the order violated
        elif kind == 3:
            w["nfree"] = nkf + 1
        elif n:
            w["pt"][n - 1] = npt                             # a point beyond pt_counts
        else:
            w["poses"][0, 3] = np.nan
    return w


def ba_item(w, st):
    return w if st[1] else {k: v for k, v in w.items() if k not in ("level", "tab")}


def ba_launch(ctx, st, items):
    ws = [ba_item(w, st) for w in items]
    return tba.Device(ctx).run(ws, st[0], tba.shape_of(ws, (0, 2, 3)))   # (kf_stride may not exceed 32)


BA = types.SimpleNamespace(
    module=tba, probe="ba_host_check", sets=BA_SETS, edits=BA_EDITS, needs={}, make=ba_make,
    lines=lambda st, items: [tba.case_line(ba_item(w, st), st[0]) for w in items],
    expect=lambda st, items: tba.probe([ba_item(w, st) for w in items], [st[0]] * len(items)),
    restate=lambda st, items, b: tba.ref_window(ba_item(items[b], st), st[0]),
    same=tba.assert_same, launch=ba_launch, check=lambda got, want, items: tba.assert_windows(got, want, items),
    codes={0, 1, 2, 3}, code=lambda w: w["status"] & 255, ran=lambda w: w["status"] & 255 == 0,
    early=lambda st, w: w["status"] >> 8 < 1 + sum(st[0][1][:st[0][0]]) + st[0][0], tied=None, sample=None,
    key=lambda w: w["poses"].tobytes() + w["xw"].tobytes(), twins=("refused",))


# ==== pislam_pose_graph_batch (and pislam_map_points_correct_batch on its result) ============================================
# iters, cg_iters, cg_tol, eps, with weights: one iteration; one conjugate-gradient iteration; a solve that stops on its
# residual test at once; the most iterations with eps 0
GRAPH_SETS = [((20, 256, 1e-6, 1e-9), False), ((1, 40, 1e-8, 1e-9), True), ((6, 1, 1e-6, 1e-9), False), ((8, 64, 0.5, 1e-9), True),
              ((64, 12, 1e-3, 0.0), True), ((6, 40, 1e-8, 1e-3), False)]
GRAPH_EDITS = ["none", "lone_vertex", "rot_min", "weights", "far_start", "all_fixed", "no_edge", "fixed_scale", "coincident", "far",
               "two_fixed", "half_turn", "refused"]


def graph_make(rng, seed, st, edit, big):
    if big:                                                  # the workgroup size in edges
        ne = around(rng, WG)
        extra = int(rng.integers(20, 80))
        nv = ne - extra
    else:
        nv = int(rng.integers(2, 25))
        extra = int(rng.integers(0, nv // 3 + 1)) if nv >= 6 else 0
    kw = dict(nv=nv, extra=extra, weights=st[1], fixed_scale=edit == "fixed_scale" or bool(rng.integers(2)),
              drift=30.0 if edit == "far_start" else float(rng.choice([0, 1, 5])))
    if edit == "two_fixed" and nv > 3:
        kw["fixed"] = (0, nv // 2)
    g = tg.make_graph(int(rng.integers(1 << 31)), **kw)
    ne = len(g["edges"])
    if edit == "lone_vertex":                                # a free vertex that no edge touches
        g = tg.graph(np.concatenate([g["sims"], g["sims"][:1]]), np.concatenate([g["fixed"], [0]]), g["edges"], g["meas"], g["weight"])
    elif edit == "rot_min":                                  # the loop edge's error a rotation with 1 + tr R at ROT_MIN
        i, j = (int(v) for v in g["edges"][ne - 1])
        th = np.arccos(tg.ROT_MIN / 2 - 1) * (1 + float(rng.choice([-1e-4, -1e-6, 0, 1e-6, 1e-4])))
        turn = tg.sim(tg.rot([0, 0, th]), [0, 0, 0], 1.0)
        g["meas"][ne - 1] = tg.sim_mul(turn, tg.rel(g["sims"][i], g["sims"][j])).astype(F32)
    elif edit == "weights":
        idx = some(rng, ne, 4)
        g["weight"][idx] = np.array([0.0, 1e30, 0.0, 1e-30], F32)[:len(idx)]
    elif edit == "all_fixed":
        g["fixed"][:] = 1
    elif edit == "no_edge":
        g = tg.graph(g["sims"], g["fixed"], np.zeros((0, 2)), np.zeros((0, 13)), np.zeros(0, F32) if st[1] else None)
    elif edit == "coincident":
        g["sims"][:] = g["sims"][0]
    elif edit == "far":                                      # the world moved some km: every measurement stays
        off = rng.choice([-1.0, 1.0], 3) * rng.uniform(2000, 6000, 3)
        for k in range(len(g["sims"])):
            S = g["sims"][k].astype(F64)
            g["sims"][k, 9:12] = (S[9:12] - S[12] * S[:9].reshape(3, 3) @ off).astype(F32)
    elif edit == "half_turn":                                # inadmissible at the input: code 2
        g["meas"][0] = tg.sim_mul(tg.sim(np.diag([-1.0, -1.0, 1.0]), [0, 0, 0], 1.0),
                                  tg.rel(g["sims"][int(g["edges"][0][0])], g["sims"][int(g["edges"][0][1])])).astype(F32)
    elif edit == "refused":
        kind = int(rng.integers(5))
        if kind == 0:
            g["sims"][int(rng.integers(len(g["sims"]))), int(rng.integers(13))] = np.nan
        elif kind == 1:
            g["meas"][int(rng.integers(ne)), 12] = F32(rng.choice([0.0, -1.0]))
        elif kind == 2:
            g["edges"][int(rng.integers(ne)), 1] = len(g["sims"])
        elif kind == 3:
            g["inc"][0] ^= 1
        else:
            g["fixed"][:] = 0
    return g


POINTS = 40


def graph_points(g):
    """Map points that refer to the graph's vertices (a few beyond them), for pislam_map_points_correct_batch."""
    nv = len(g["sims"])
    rng = np.random.default_rng([7, nv, len(g["edges"])])
    return rng.integers(0, nv + 2, POINTS).astype(np.uint16), rng.uniform(-6, 6, (POINTS, 3)).astype(F32)


def graph_expect(st, items):
    """The probe's graphs, and its corrected map points from each graph's input to its optimised similarities."""
    want = tg.probe(items, [st[0]] * len(items))
    got = tg.run_probe([tg.points_line(g["sims"], w["sims"], *graph_points(g)) for g, w in zip(items, want)])
    for w, ln in zip(want, got):
        t = np.array(ln.split()).reshape(-1, 4)
        w["pts"], w["pts_status"] = words(t[:, 1:].reshape(-1)).reshape(-1, 3), np.array([int(x) for x in t[:, 0]], np.uint8)
    return want


def graph_restate(st, items, b):
    r = tg.ref_graph(items[b], st[0])
    r["pts"], r["pts_status"] = tg.ref_correct_points(items[b]["sims"], r["sims"], *graph_points(items[b]))
    return r


def graph_same(got, want, tag):
    tg.assert_same(got, want, tag)
    assert tg.bits(got["pts"]) == tg.bits(want["pts"]) and got["pts_status"].tolist() == want["pts_status"].tolist(), tag


def graph_launch(ctx, st, items):
    """The graphs, then the map points from the input to the output similarities, which stay on the device."""
    d = tg.Device(ctx)
    t, ptr, B, shape = d.torch, d.capi.ptr, len(items), tg.shape_of(items, (1, 2))
    dev = d.upload(d.pack(items, *shape, weighted=st[1]))
    o = d.sentinels(B, shape[0])
    assert d.call(st[0], dev, shape, B, o) == 0, d.lib.pislam_last_error(ctx.h)
    ctx.synchronize()
    pts = [graph_points(g) for g in items]
    xw, ref = d.up(np.stack([p[1] for p in pts])), d.up(np.stack([p[0] for p in pts]).view(np.int16))
    cnt = d.up(np.full(B, POINTS, np.int32))
    out = t.full((B, POINTS, 3), tg.SENT, dtype=t.int32, device="cuda").view(t.float32)
    status = t.full((B, POINTS), 0xA5, dtype=t.uint8, device="cuda")
    assert d.lib.pislam_map_points_correct_batch(ctx.h, ptr(xw), ptr(ref), ptr(cnt), ptr(dev["sims"]), ptr(o["sims_out"]),
                                                 ptr(dev["v_counts"]), POINTS, shape[0], B, ptr(out), ptr(status)) == 0
    ctx.synchronize()
    return dict({k: v.cpu().numpy() for k, v in o.items()}, pts=out.cpu().numpy(), pts_status=status.cpu().numpy())


def graph_check(got, want, items):
    tg.assert_graphs(got, want, items)
    for b, w in enumerate(want):
        assert tg.bits(got["pts"][b]) == tg.bits(w["pts"]) and got["pts_status"][b].tolist() == w["pts_status"].tolist(), (
            "graph %d: corrected map points" % b)


GRAPH = types.SimpleNamespace(
    module=tg, probe="graph_host_check", sets=GRAPH_SETS, edits=GRAPH_EDITS, needs={"weights": lambda st: st[1]}, make=graph_make,
    lines=lambda st, items: [tg.case_line(g, st[0]) for g in items], expect=graph_expect, restate=graph_restate,
    same=graph_same, launch=graph_launch, check=graph_check,
    codes={0, 1, 2, 3}, code=lambda w: w["status"] & 255, ran=lambda w: w["status"] & 255 == 0 and w["status"] >> 8 > 0,
    early=lambda st, w: w["status"] >> 8 < 1 + st[0][0], tied=None, key=lambda w: w["sims"].tobytes() + np.array(w["cost"]).tobytes(),
    twins=("refused", "all_fixed", "no_edge", "half_turn", "coincident"),
    sample=lambda g: len(g["sims"]) <= 40)               # the restatement is slow: graphs of a few dozen vertices


# ==== pislam_pnp_ransac_batch ===============================================================================================
# hypotheses, seed, min_inliers, with levels: every hypothesis count of the issue; a min_inliers above every count
PNP_SETS = [(64, 5, 10, True), (1, 7, 4, False), (63, 11, 10, True), (65, 3, 16384, False), (HYPOTHESES[4], 9, 10, True),
            (64, 0xFFFFFFFF, 4, False)]
RANSAC_EDITS = ["none", "depth", "far", "plane", "line", "focal_small", "focal_large", "outliers", "ties", "q8", "level", "few",
                "identical", "refused"]


def mirrored_twice(a, sign):
    """a, a again, and both mirrored by `sign` (a per-column factor, or a function of the array)."""
    m = sign(a) if callable(sign) else a * sign
    return np.concatenate([a, a, m, m]).astype(a.dtype)


def pnp_make(rng, seed, st, edit, big):
    n = around(rng, WG_RANSAC) if big else int(rng.integers(4, 65))
    if edit == "few":
        n = int(rng.integers(0, 4))
    if edit == "ties" and not big:
        n = int(rng.integers(1, 5)) * 4                      # a few distinct points, each four times
    fr, truth, _ = tpnp.scene(int(rng.integers(1 << 31)), n=n, outliers=0.5 if edit == "outliers" else float(rng.choice([0, 0.2, 0.4])),
                              levels=True, scale=float(rng.choice([1.0, 1.0, 0.01, 100.0])))
    cx = float(fr["cam"][2])
    if edit == "depth":
        idx = some(rng, n, 4)
        fr["xw"][idx, 2] = np.array([0, tpose.Z_MIN, np.nextafter(tpose.Z_MIN, F32(0)), -1], F32)[:len(idx)]
    elif edit == "far":                                      # the world some km away: the pose that explains it moves along
        fr["xw"] = (fr["xw"].astype(F64) + rng.choice([-1.0, 1.0], 3) * rng.uniform(2000, 6000, 3)).astype(F32)
    elif edit == "plane":
        fr["xw"][:, 2] = 6
        fr["obs"] = observe(fr["xw"], truth, fr["cam"], fr["obs"])
    elif edit == "line":
        fr["xw"] = on_a_line(rng, n)
        fr["obs"] = observe(fr["xw"], truth, fr["cam"], fr["obs"])
    elif edit in ("focal_small", "focal_large"):
        fr["cam"][:2] *= F32(0.01 if edit == "focal_small" else 50)
    elif edit == "ties":                                     # every observation twice and the set mirrored in x: equal scores
        q = n // 4
        fr["xw"] = mirrored_twice(fr["xw"][:q], np.array([-1, 1, 1], F32))
        fr["obs"] = mirrored_twice(fr["obs"][:q], lambda o: np.stack([int(round(2 * cx * 256)) - o[:, 0], o[:, 1], o[:, 2]], 1))
        fr["level"] = mirrored_twice(fr["level"][:q], 1)
        n = 4 * q
        fr = tpnp.sub(fr, n)
    elif edit == "q8":
        idx = some(rng, n, 4)
        fr["obs"][idx] = Q8_EXTREMES[:len(idx)]
    elif edit == "level":
        idx = some(rng, n, 3)
        fr["level"][idx] = np.array([4, 5, 255], np.uint8)[:len(idx)]
    elif edit == "identical":                                # one point n times: no sample has a solution
        fr["xw"][:], fr["obs"][:] = fr["xw"][:1], fr["obs"][:1]
    elif edit == "refused":
        if rng.integers(2):
            fr["cam"][int(rng.integers(5))] = F32(rng.choice([np.nan, np.inf]))
        else:
            fr["cam"][int(rng.integers(2))] = 0
    return fr


def pnp_item(fr, st):
    return fr if st[3] else dict(fr, level=None, tab=None)


def pnp_launch(ctx, st, items):
    ns = [len(fr["obs"]) for fr in items]
    return tpnp.Device(ctx).run([pnp_item(fr, st) for fr in items], ns, max(ns) + 1, st[:3], st[3])


def pnp_tied(st, items, b):
    hyp = tpnp.ref_hypotheses(pnp_item(items[b], st), st[1], b, st[0])
    return hyp is not None and int(hyp["score"].max()) > 0 and int((hyp["score"] == hyp["score"].max()).sum()) >= 2


def ransac_row(**kw):
    return types.SimpleNamespace(codes={0, 1, 2, 3}, code=lambda w: w["status"] & 255, ran=lambda w: w["best"] >= 0, early=None,
                                 twins=("refused", "few", "identical", "ties"), sample=None, **kw)


PNP = ransac_row(
    module=tpnp, probe="pnp_host_check", sets=PNP_SETS, edits=RANSAC_EDITS, needs={}, make=pnp_make,
    lines=lambda st, items: [tpnp.probe_line(pnp_item(fr, st), b, *st[:3]) for b, fr in enumerate(items)],
    parse=lambda st, items, got: [tpnp.parse_result(g, len(fr["obs"])) for g, fr in zip(got, items)],
    restate=lambda st, items, b: tpnp.ref_frame(pnp_item(items[b], st), b, *st[:3]),
    same=same_by_line(tpnp.result_line), launch=pnp_launch,
    check=lambda got, want, items: tpnp.assert_frames(got, want, [len(fr["obs"]) for fr in items]),
    tied=pnp_tied, key=lambda w: w["pose"].tobytes() + bytes(str(w["score"]), "ascii"))


# ==== pislam_sim3_ransac_batch ==============================================================================================
# hypotheses, seed, min_inliers, fixed_scale, with levels
SIM3_SETS = [(64, 5, 20, 0, True), (1, 7, 3, 1, False), (63, 11, 10, 0, True), (65, 3, 16384, 0, False),
             (HYPOTHESES[4], 9, 20, 1, True), (64, 0xFFFFFFFF, 3, 0, False)]
SIM3_EDITS = [e if e != "far" else "coincident" for e in RANSAC_EDITS]


def sim3_make(rng, seed, st, edit, big):
    n = around(rng, WG_RANSAC) if big else int(rng.integers(3, 65))
    if edit == "few":
        n = int(rng.integers(0, 3))
    if edit == "ties" and not big:
        n = int(rng.integers(1, 5)) * 4
    pr, truth, _ = tsim.scene(int(rng.integers(1 << 31)), n=n, outliers=0.5 if edit == "outliers" else float(rng.choice([0, 0.2, 0.4])),
                              levels=True, fixed_scale=bool(st[3]))
    pr = pair_edit(rng, pr, truth, edit, n)
    if edit == "ties":                                       # every match twice and the set mirrored in x on both sides
        q = n // 4
        flip = lambda cam: (lambda o: np.stack([int(round(2 * float(cam[2]) * 256)) - o[:, 0], o[:, 1], o[:, 2]], 1))
        for k, sign in (("x1", np.array([-1, 1, 1], F32)), ("x2", np.array([-1, 1, 1], F32)), ("obs1", flip(pr["cam1"])),
                        ("obs2", flip(pr["cam2"])), ("level1", 1), ("level2", 1)):
            pr[k] = mirrored_twice(pr[k][:q], sign)
    elif edit == "identical":
        for k in PAIR_KEYS:
            pr[k][:] = pr[k][:1]
    elif edit == "refused":
        cam = pr["cam%d" % (1 + int(rng.integers(2)))]
        if rng.integers(2):
            cam[int(rng.integers(5))] = F32(rng.choice([np.nan, np.inf]))
        else:
            cam[int(rng.integers(2))] = 0
    return pr


def sim3_item(pr, st):
    return pr if st[4] else tsim.no_levels(pr)


def sim3_launch(ctx, st, items):
    ns = [len(pr["obs1"]) for pr in items]
    return tsim.Device(ctx).run([sim3_item(pr, st) for pr in items], ns, max(ns) + 1, st[:4], st[4])


def sim3_tied(st, items, b):
    hyp = tsim.ref_hypotheses(sim3_item(items[b], st), st[1], b, bool(st[3]), st[0])
    return hyp is not None and int(hyp["score"].max()) > 0 and int((hyp["score"] == hyp["score"].max()).sum()) >= 2


SIM3 = ransac_row(
    module=tsim, probe="sim3_host_check", sets=SIM3_SETS, edits=SIM3_EDITS, needs={}, make=sim3_make,
    lines=lambda st, items: [tsim.probe_line(sim3_item(pr, st), b, *st[:4]) for b, pr in enumerate(items)],
    parse=lambda st, items, got: [tsim.parse_result(g, len(pr["obs1"])) for g, pr in zip(got, items)],
    restate=lambda st, items, b: tsim.ref_pair(sim3_item(items[b], st), b, st[0], st[1], st[2], bool(st[3])),
    same=same_by_line(tsim.result_line), launch=sim3_launch,
    check=lambda got, want, items: tsim.assert_pairs(got, want, [len(pr["obs1"]) for pr in items]),
    tied=sim3_tied, key=lambda w: w["sim"].tobytes() + bytes(str(w["score"]), "ascii"))


# ==== pislam_two_view_ransac_batch (F and H) ==================================================================================
# model, hypotheses, seed, sigma_q8
TV_SETS = [(ttv.FUND, 64, 12345, 256), (ttv.HOMOG, 64, 7, 256), (ttv.FUND, 1, 3, 1), (ttv.HOMOG, 63, 5, 4096), (ttv.FUND, 65, 9, 256),
           (ttv.HOMOG, HYPOTHESES[4], 11, 256)]
TV_EDITS = ["none", "other_geometry", "outliers", "zero_baseline", "collinear", "ties", "extremes", "noise_free", "duplicate", "tiny",
            "refused"]


def tv_make(rng, seed, st, edit, big):
    m = ttv.SAMPLE[st[0]]
    n = around(rng, WG_RANSAC) if big else int(rng.integers(m, 65))
    plane = (st[0] == ttv.HOMOG) != (edit == "other_geometry")   # a plane for F, depth for H: the other model's scene
    u, v, _ = ttv.scene(int(rng.integers(1 << 31)), plane, n=n, outliers=0.5 if edit == "outliers" else float(rng.choice([0, 0.2])),
                        noise=0.0 if edit == "noise_free" else 0.5)
    if edit == "zero_baseline":
        v = u.copy()
    elif edit == "collinear":
        u, v = ttv.collinear(n, int(rng.integers(1 << 31)))
    elif edit == "ties":                                     # every match twice and the set mirrored in x: equal scores
        q = max(n // 4, 2)
        flip = lambda p: np.stack([640 * 256 - p[:, 0], p[:, 1]], 1)
        u, v = mirrored_twice(u[:q], flip), mirrored_twice(v[:q], flip)
    elif edit == "extremes":                                 # a third of the scene beyond +- 2^20, and the boundary itself
        u, v = (u - 320 * 256) * 9, (v - 320 * 256) * 9
        u[0], v[1] = (1 << 20, -(1 << 20)), ((1 << 20) + 1, -(1 << 20) - 1)
        u[2], v[3] = (1 << 30, 5), (-(1 << 31), (1 << 31) - 1)
    elif edit == "duplicate":
        u, v = twice(u, n), twice(v, n)
    elif edit == "tiny":                                     # the whole scene inside a few Q8 units
        u, v = u // 4096 + 100 * 256, v // 4096 + 100 * 256
    elif edit == "refused":                                  # nothing is evaluated: too few, or one image's points all equal
        if rng.integers(2):
            u, v = u[:int(rng.integers(0, m))], v[:int(rng.integers(0, m))]
            u, v = u[:min(len(u), len(v))], v[:min(len(u), len(v))]
        else:
            u[:] = u[0]
    return dict(u=np.asarray(u, np.int64), v=np.asarray(v, np.int64))


def tv_lines(st, items):
    return [" ".join(str(x) for x in list(st) + [b, len(it["u"])] + np.concatenate([it["u"], it["v"]], 1).astype(np.int32).ravel().tolist())
            for b, it in enumerate(items)]


def tv_parse(st, items, got):
    out = []
    for g in got:
        t = g.split()
        out.append(dict(best=int(t[0]), score=int(t[1]), ninliers=int(t[2]), inlier=bits_of(t[3]), model_n=words(t[4:13]),
                        stats=np.array([int(x) for x in t[13:21]], np.int64)))
    return out


def tv_line(r):
    return " ".join([str(int(r["best"])), str(int(r["score"])), str(int(r["ninliers"])), "".join(str(int(x)) for x in r["inlier"]) or "-"]
                    + ["%08x" % int(x) for x in np.asarray(r["model_n"], F32).view(np.uint32)] + [str(int(x)) for x in r["stats"]])


def tv_pack(items):
    B, stride = len(items), max(len(it["u"]) for it in items) + 1
    rng = np.random.default_rng(77)
    p1, p2 = (rng.integers(-(1 << 31), 1 << 31, (B, stride, 2)).astype(np.int64) for _ in range(2))
    for b, it in enumerate(items):
        n = len(it["u"])
        p1[b, :n], p2[b, :n] = it["u"], it["v"]
    return p1, p2, np.array([len(it["u"]) for it in items], np.int64)


def tv_check(got, want, items):
    B, stride = got["inlier"].shape
    w = dict(best=np.array([x["best"] for x in want], np.int32), score=np.array([x["score"] for x in want], np.uint32),
             ninliers=np.array([x["ninliers"] for x in want], np.uint32), inlier=np.full((B, stride), ttv.SENT8, np.uint8),
             model_n=np.stack([x["model_n"] for x in want]), stats=np.stack([x["stats"] for x in want]))
    for b, x in enumerate(want):
        w["inlier"][b, :len(x["inlier"])] = x["inlier"]
    ttv.assert_same(got, w)


def tv_tied(st, items, b):
    """The module's restatement, hypothesis by hypothesis, with the scores kept."""
    model, hypotheses, seed, sigma = st
    stats, pts = ttv.ref_stats(items[b]["u"].tolist(), items[b]["v"].tolist())
    n = stats[0]
    if n < ttv.SAMPLE[model] or stats[3] == 0 or stats[6] == 0:
        return False
    scores = []
    with np.errstate(all="ignore"):
        X, w1, w2 = ttv.ref_normalise(stats, pts, sigma)
        for k in range(hypotheses):
            f = ttv.ref_solve(ttv.ref_rows(model, X, ttv.ref_sample(seed, b, k, n, ttv.SAMPLE[model])))
            scores.append(0 if f is None else ttv.ref_score(model, f, X, w1, w2)[0])
    return max(scores) > 0 and scores.count(max(scores)) >= 2


TWO_VIEW = types.SimpleNamespace(
    module=ttv, probe="ransac_host_check", sets=TV_SETS, edits=TV_EDITS, needs={}, make=tv_make, lines=tv_lines, parse=tv_parse,
    restate=lambda st, items, b: ttv.ref_pair(items[b]["u"].tolist(), items[b]["v"].tolist(), b, *st), same=same_by_line(tv_line),
    launch=lambda ctx, st, items: ttv.Device(ctx).run(*tv_pack(items), *st), check=tv_check,
    codes={0, 1}, code=lambda w: int(w["best"] >= 0), ran=lambda w: w["best"] >= 0, early=None, tied=tv_tied,
    key=lambda w: w["model_n"].tobytes() + bytes(str(w["score"]), "ascii"),
    twins=("refused", "ties", "collinear", "zero_baseline"),
    sample=lambda it: len(it["u"]) <= 64)                    # the restatement loops over the hypotheses in Python


# ==== pislam_two_view_reconstruct_batch =======================================================================================
# (sigma_q8, cos_parallax, cos_point, min_good, min_good_pct, similar_pct, parallax_rank), ncand, with a mask
RC_EASY = (256, trec.COS_1DEG, F32(0.99998), 5, 90, 70, 6)
RC_SETS = [(RC_EASY, 4, False), (trec.LOOSE, 4, True), (RC_EASY, 1, False), (trec.DEFAULT, 8, True),
           ((4096, F32(0.9999), F32(0.99998), 3, 100, 99, 3), 4, False), ((1, F32(1.0), F32(1.0), 1, 0, 100, 1), 2, True)]
RC_EDITS = ["none", "far_points", "tiny_baseline", "spoiled", "ambiguous", "plane", "focal_small", "focal_large", "cand_nan", "extremes",
            "masked", "few", "refused"]


def rc_make(rng, seed, st, edit, big):
    n = around(rng, WG_RECON) if big else int(rng.integers(3, 65))
    if edit == "few":
        n = int(rng.integers(0, 3))
    first = int(rng.integers(min(4, st[1])))                 # the truth is among the candidates of the call
    cam = trec.CAM * F32(rng.choice([1.0, 0.8, 1.3]))
    if edit in ("focal_small", "focal_large"):               # the scene is seen through this camera
        cam[:2] *= F32(0.01 if edit == "focal_small" else 50)
    kw = dict(far=n // 4 + 1 if edit == "far_points" and n else 0, baseline=1e-3 if edit == "tiny_baseline" else float(rng.choice([0.2, 0.5, 1.0])),
              depth=(6.0, 6.0) if edit == "plane" else (4.0, 8.0), rot_deg=float(rng.choice([0.0, 2.0, 6.0])), cam=cam)
    sc = trec.scene(int(rng.integers(1 << 31)), n, **kw)
    if edit == "spoiled":
        sc = trec.spoil(sc, np.arange(0, n, int(rng.choice([2, 20]))))
    it = dict(q1=sc["q1"], q2=sc["q2"], cam=cam.copy(), cand=trec.eight_motions(sc, seed, first=first),
              mask=(rng.random(n) < 0.8).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8))
    if edit == "ambiguous":                                  # the truth twice: the second best is as good as the best
        it["cand"][(first + 1) % 4] = it["cand"][first]
    elif edit == "cand_nan":                                 # one candidate, or all of them
        which = slice(None) if rng.random() < 0.25 else (first + 2) % 4
        it["cand"][which, int(rng.integers(12))] = np.nan
    elif edit == "extremes":
        idx = some(rng, n, 4)
        it["q1"][idx] = np.array([[1 << 20, -(1 << 20)], [(1 << 20) + 1, -(1 << 20) - 1], [1 << 30, 5], [-(1 << 31), (1 << 31) - 1]])[:len(idx)]
    elif edit == "masked":                                   # every second match, or all of them
        it["mask"][::1 if rng.random() < 0.25 else 2] = 0
    elif edit == "refused":
        if rng.integers(2):
            it["cam"][int(rng.integers(4))] = F32(rng.choice([np.nan, np.inf]))
        else:
            it["cam"][int(rng.integers(2))] = 0
    return it


def rc_parse(st, items, got):
    """The probe's lines as one-pair results of the module's ref_batch."""
    out = []
    for g, it in zip(got, items):
        t, n = g.split(), len(it["q1"])
        S = max(n, 1)
        r = dict(best=np.array([int(t[0])], np.int32), status=np.array([int(t[1])], np.uint32),
                 ngood=np.array([[int(x) for x in t[2:10]]], np.uint32), npar=np.array([[int(x) for x in t[10:18]]], np.uint32),
                 pose_out=words(t[18:30])[None], xw=np.full((1, S, 3), trec.SENT32, np.uint32).view(F32),
                 point=np.full((1, S), trec.SENT8, np.uint8), n=np.array([n]))
        r["point"][0, :n] = bits_of(t[30])
        if n:
            r["xw"][0, :n] = words(t[31:31 + 3 * n]).reshape(n, 3)
        out.append(r)
    return out


def rc_restate(st, items, b):
    it = items[b]
    n = len(it["q1"])
    pad = lambda a, shape: np.concatenate([a, np.zeros(shape, a.dtype)]) if n == 0 else a
    return trec.ref_batch(pad(it["q1"], (1, 2))[None], pad(it["q2"], (1, 2))[None], [n], pad(it["mask"], 1)[None] if st[2] else None,
                          it["cam"][None], it["cand"][None, :st[1]], st[0])


def rc_pack(st, items):
    B, stride = len(items), max(len(it["q1"]) for it in items) + 1
    rng = np.random.default_rng(17)
    q1, q2 = (rng.integers(-1 << 31, 1 << 31, (B, stride, 2)) for _ in range(2))
    mask = rng.integers(0, 256, (B, stride)).astype(np.uint8)
    for b, it in enumerate(items):
        n = len(it["q1"])
        q1[b, :n], q2[b, :n], mask[b, :n] = it["q1"], it["q2"], it["mask"]
    return (q1, q2, np.array([len(it["q1"]) for it in items], np.uint32), mask if st[2] else None,
            np.stack([it["cam"] for it in items]).astype(F32), np.stack([it["cand"][:st[1]] for it in items]).astype(F32), st[0])


def rc_check(got, want, items):
    B, stride = got["point"].shape
    w = {k: np.concatenate([x[k] for x in want]) for k in ("best", "status", "ngood", "npar", "pose_out")}
    w["xw"], w["point"] = np.full((B, stride, 3), trec.SENT32, np.uint32).view(F32), np.full((B, stride), trec.SENT8, np.uint8)
    for b, (x, it) in enumerate(zip(want, items)):
        n = len(it["q1"])
        w["xw"][b, :n], w["point"][b, :n] = x["xw"][0, :n], x["point"][0, :n]
    trec.assert_same(got, w)


RECON = types.SimpleNamespace(
    module=trec, probe="recon_host_check", sets=RC_SETS, edits=RC_EDITS, needs={}, make=rc_make,
    lines=lambda st, items: [trec.probe_line(it["q1"], it["q2"], len(it["q1"]), it["mask"] if st[2] else None, it["cam"], it["cand"][:st[1]], st[0])
                             for it in items],
    parse=rc_parse, restate=rc_restate, same=same_by_line(lambda r: trec.result_line(r, 0)),
    launch=lambda ctx, st, items: trec.Device(ctx).run(*rc_pack(st, items)), check=rc_check,
    codes={0, 1, 2, 3, 4}, code=lambda w: int(w["status"][0]) & 255, ran=lambda w: int(w["status"][0]) & 255 == 0, early=None, tied=None,
    key=lambda w: w["xw"].tobytes() + w["pose_out"].tobytes(), twins=("refused", "few"), sample=None)


# ==== pislam_triangulate_batch ==================================================================================================
# levels, scale factor, parameters other than the module's PAR
TRI_SETS = [(8, 1.2, ()), (8, 1.2, (("cos_min_parallax", 2.0),)), (1, 1.5, ()), (5, 1.1, (("ratio_factor", 1.2),)),
            (8, 1.2, (("chi2_mono", 0.5), ("chi2_stereo", 0.5)))]
TRI_EDITS = ["none", "same_place", "parallel", "ahead", "focal_small", "focal_large", "far", "q8", "level", "mono_only", "duplicate",
             "refused"]
TRI_SLOT = ("obs1", "obs2", "l1", "l2")


def tri_make(rng, seed, st, edit, big):
    n = around(rng, WG_TRI) if big else int(rng.integers(1, 65))
    pose1, pose2, cam1, cam2 = ttri.random_pair(rng, dict(same_place=1, parallel=2, ahead=3).get(edit, 0))
    if edit in ("focal_small", "focal_large"):
        cam1[:2] *= F32(0.01 if edit == "focal_small" else 50)
    elif edit == "mono_only":
        cam1[4] = cam2[4] = 0
    elif edit == "far":                                      # both key frames some km from the origin
        off = rng.choice([-1.0, 1.0], 3) * rng.uniform(2000, 6000, 3)
        for p in (pose1, pose2):
            p[9:] = (p[9:].astype(F64) - p[:9].reshape(3, 3).astype(F64) @ off).astype(F32)
    q1, q2, l1, l2 = ttri.random_slots(rng, pose1, pose2, cam1, cam2, n, st[0])
    it = dict(pose1=pose1, pose2=pose2, cam1=cam1, cam2=cam2, obs1=q1, obs2=q2, l1=l1, l2=l2)
    if edit == "parallel":                                   # one pixel from one place through one camera: the rays never meet
        it["cam2"], it["obs1"][:, 2] = cam1.copy(), MONO
        it["obs2"] = it["obs1"].copy()
    if edit == "q8":
        idx = some(rng, n, 4)
        it["obs1"][idx] = Q8_EXTREMES[:len(idx)]
        idx = some(rng, n, 2)
        it["obs2"][idx] = Q8_EXTREMES[2:2 + len(idx)]
    elif edit == "level":
        idx = some(rng, n, 3)
        it["l1"][idx] = np.array([st[0], st[0] + 1, 255])[:len(idx)]
        idx = some(rng, n, 2)
        it["l2"][idx] = np.array([255, st[0]])[:len(idx)]
    elif edit == "duplicate":
        for k in TRI_SLOT:
            it[k] = twice(it[k], n)
    elif edit == "refused":
        if rng.integers(2):
            it["pose%d" % (1 + int(rng.integers(2)))][int(rng.integers(12))] = F32(rng.choice([np.nan, np.inf, -np.inf]))
        else:
            it["cam%d" % (1 + int(rng.integers(2)))][int(rng.integers(2))] = 0
    return it


def tri_tables(st):
    ls, sg = ttri.level_tables(st[0], st[1])
    return dict(ls=ls, sg=sg)


def tri_lines(st, items):
    """One line per slot."""
    return [ttri.probe_line(dict({k: it[k] for k in ("pose1", "pose2", "cam1", "cam2")}, obs1=it["obs1"][i].tolist(), obs2=it["obs2"][i].tolist(),
                                 l1=int(it["l1"][i]), l2=int(it["l2"][i]), **tri_tables(st), **dict(st[2])))
            for it in items for i in range(len(it["obs1"]))]


def tri_parse(st, items, got):
    out, at = [], 0
    for it in items:
        n = len(it["obs1"])
        t = np.array([g.split() for g in got[at:at + n]]).reshape(n, 10)
        at += n
        w = words(t[:, 2:].reshape(-1)).reshape(n, 8)
        out.append(dict(status=t[:, 0].astype(np.uint8), mode=t[:, 1].astype(np.uint8), xw=w[:, :3], normal=w[:, 3:6], drange=w[:, 6:]))
    return out


def tri_restate(st, items, b):
    it = items[b]
    return ttri.ref_pair(it["pose1"], it["pose2"], it["cam1"], it["cam2"], it["obs1"], it["obs2"], it["l1"], it["l2"], **tri_tables(st), **dict(st[2]))


def tri_same(got, want, tag):
    for k in ("status", "mode", "xw", "normal", "drange"):
        g, w = (np.ascontiguousarray(x[k]) for x in (got, want))
        assert (g.view(np.uint32) == w.view(np.uint32)).all() if g.dtype == F32 else (g == w).all(), (tag, k)


def tri_launch(ctx, st, items):
    B, stride = len(items), max(len(it["obs1"]) for it in items) + 1
    rng = np.random.default_rng(41)
    c = dict(obs1=rng.integers(-1 << 31, 1 << 31, (B, stride, 3)).astype(np.int32), obs2=rng.integers(-1 << 31, 1 << 31, (B, stride, 3)).astype(np.int32),
             l1=rng.integers(0, 256, (B, stride)).astype(np.uint8), l2=rng.integers(0, 256, (B, stride)).astype(np.uint8),
             counts=np.array([len(it["obs1"]) for it in items], np.uint32), **tri_tables(st))
    for k in ("pose1", "pose2", "cam1", "cam2"):
        c[k] = np.stack([it[k] for it in items]).astype(F32)
    for b, it in enumerate(items):
        n = len(it["obs1"])
        for k in TRI_SLOT:
            c[k][b, :n] = it[k]
    return ttri.run_triangulate(ctx, c, **dict(st[2]))


def tri_check(got, want, items):
    B, stride = got[1].shape
    xw, normal = np.full((B, stride, 3), ttri.SF, F32), np.full((B, stride, 3), ttri.SF, F32)
    drange, status = np.full((B, stride, 2), ttri.SF, F32), np.full((B, stride), ttri.S8, np.uint8)
    npoints = np.zeros(B, np.uint32)
    for b, x in enumerate(want):
        n = len(x["status"])
        xw[b, :n], normal[b, :n], drange[b, :n], status[b, :n] = x["xw"], x["normal"], x["drange"], x["status"]
        npoints[b] = int((x["status"] == ttri.OK).sum())
    ttri.assert_outputs(got, (xw, status, normal, drange, npoints))


TRIANGULATE = types.SimpleNamespace(
    module=ttri, probe="mappoint_host_check", sets=TRI_SETS, edits=TRI_EDITS,
    needs={"parallel": lambda st: dict(st[2]).get("cos_min_parallax") == 2.0}, make=tri_make, lines=tri_lines, parse=tri_parse,
    restate=tri_restate, same=tri_same, launch=tri_launch, check=tri_check,
    codes=set(range(10)), code=lambda w: set(int(x) for x in w["status"]), ran=lambda w: bool((w["status"] == ttri.OK).any()),
    early=None, tied=None, key=lambda w: w["xw"].tobytes(), twins=("refused", "duplicate"), sample=None)


# ==== pislam_covisibility_batch ===============================================================================================
# min_weight, cull_min_observers, cull_level_slack, nb_stride, with levels, with a mask: ORB-SLAM's; every link and a row cut
# to 3; no levels and every level passing; rows as long as the key frames; a min_weight above every weight (the fallback);
# one neighbour
CV_SETS = [(15, 3, 1, 8, True, True), (1, 3, 0, 3, True, False), (2, 1, 255, 64, False, True), (1, 2, 1, 300, True, True),
           (100000, 3, 1, 5, False, False), (3, 5, 0, 1, True, True)]
CV_EDITS = ["none", "equal_weights", "spare", "path", "mask_none", "levels_extreme", "one_point", "empty", "no_key_frames",
            "lone_observers", "refused"]


def cv_make(rng, seed, st, edit, big):
    nk = around(rng, 64, WG_COVIS) if big else int(rng.integers(1, 11))
    s = int(rng.integers(1 << 31))
    if edit == "equal_weights":                              # the sort key and the parent rule decide by index alone
        m = tcov.clique_map(nk, int(rng.integers(1, 4))) if big or rng.integers(2) else tcov.pairs_map(nk, int(rng.integers(1, 3)))
    elif edit == "path" and nk >= 3:
        m = tcov.path_map(s, nk, points=4 * nk if big else min(4 * nk, 20), run=int(rng.integers(2, 4)))
    elif edit == "one_point":
        m = tcov.clique_map(nk, 1)
    elif edit == "lone_observers":                           # every point has one observer: no weight at all
        m = tcov.make_map({3 * p: {int(rng.integers(nk))} for p in range(2 * nk)}, nk, rng, levels=True, mask=True)
    else:
        m = tcov.random_map(s, nk, extra=int(rng.integers(0, nk // 3 + 1)))
    n = len(m["pt"])
    m.setdefault("level", rng.integers(0, 8, n).astype(np.uint8))
    m.setdefault("mask", (rng.random(n) < 0.7).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8))
    m["ks"] = m["nk"]
    if edit == "spare":
        m["nk"] = m["ks"] = nk + 3
    elif edit == "mask_none":
        m["mask"][:] = 0
    elif edit == "levels_extreme":
        m["level"] = rng.choice(np.array([0, 254, 255], np.uint8), n)
    elif edit == "empty":
        m["count"] = 0
    elif edit == "no_key_frames":
        m = dict(m, nk=0, count=0)
    elif edit == "refused" and n:
        kind = int(rng.integers(5))
        if kind == 0 and n >= 2:
            m["pt"][[0, n - 1]] = m["pt"][[n - 1, 0]]        # a descending obs_pt
        elif kind == 1:
            m["kf"][int(rng.integers(n))] = nk               # obs_kf == nk
        elif kind == 2:
            m["pt"][0] = -1
        elif kind == 3:
            m["count"] = -1
        else:
            m["nk"] = -2
    return m


def cv_batch(st, items):
    return tcov.batch_of(items, pad=(3, 2), level=st[4], mask=st[5])


def cv_rows(st, bt):
    return min(st[3], bt["ks"])                              # nb_stride may not exceed kf_stride


def cv_split(r, B):
    return [{k: np.asarray(r[k])[b:b + 1] for k in tcov.NAMES} for b in range(B)]


def cv_restate(st, items, b):
    bt = cv_batch(st, items)
    r = tcov.ref_map(bt["pt"][b], bt["kf"][b], None if bt["level"] is None else bt["level"][b], None if bt["mask"] is None else bt["mask"][b],
                     int(bt["counts"][b]), int(bt["nk"][b]), bt["ks"], st[:3], cv_rows(st, bt))
    return {k: np.asarray(r[k])[None] for k in tcov.NAMES}


def cv_expect(st, bt):
    return cv_split(tcov.probe(bt, st[:3], cv_rows(st, bt)), len(bt["counts"]))


def cv_launch(ctx, st, bt):
    return tcov.gpu(ctx, bt, st[:3], cv_rows(st, bt))


def cv_lines(st, items):
    return [" ".join("%s=%s" % (k, np.asarray(m[k]).tolist()) for k in sorted(m)) for m in items]


COVIS = types.SimpleNamespace(
    module=tcov, probe="covis_host_check", sets=CV_SETS, edits=CV_EDITS, needs={}, make=cv_make, lines=cv_lines,
    expect=lambda st, items: cv_expect(st, cv_batch(st, items)), restate=cv_restate,
    same=tcov.assert_same, launch=lambda ctx, st, items: cv_launch(ctx, st, cv_batch(st, items)),
    check=lambda got, want, items: tcov.assert_same(got, {k: np.concatenate([w[k] for w in want]) for k in tcov.NAMES}, "covisibility"),
    codes={0, 1, 3}, code=lambda w: int(w["status"][0]), ran=lambda w: int(w["status"][0]) == 0, early=None, tied=None,
    key=lambda w: w["nb_weight"].tobytes() + w["nb_idx"].tobytes() + w["kf_points"].tobytes() + w["kf_redundant"].tobytes(),
    twins=("refused", "equal_weights", "one_point", "lone_observers", "empty", "no_key_frames", "mask_none"), sample=None)


ROWS = dict(pose=POSE, sim3_refine=REFINE, local_ba=BA, pose_graph=GRAPH, pnp=PNP, sim3=SIM3, two_view=TWO_VIEW, reconstruct=RECON,
            triangulate=TRIANGULATE, covisibility=COVIS)
KERNELS = list(ROWS)


# ---- the generator and the comparison ------------------------------------------------------------------------------------------
def case(kernel, seed):
    """The case (kernel, seed): dict(kernel, seed, set: the index of its parameter set, edit, big, item)."""
    row = ROWS[kernel]
    rng = np.random.default_rng([KERNELS.index(kernel), seed])
    edit = row.edits[seed % len(row.edits)]
    big = bool(rng.random() < 0.25)
    sets = [s for s in range(len(row.sets)) if row.needs.get(edit, lambda st: True)(row.sets[s])]
    s = sets[int(rng.integers(len(sets)))]
    return dict(kernel=kernel, seed=seed, set=s, edit=edit, big=big, item=row.make(rng, seed, row.sets[s], edit, big))


def tag(c):
    return "(%s, seed %d, parameter set %d %r, edit %s)" % (c["kernel"], c["seed"], c["set"], ROWS[c["kernel"]].sets[c["set"]], c["edit"])


def batches(kernel, seeds):
    """The cases of the seeds as batches: [(set index, [case, ...] in the order of the seeds)], one per parameter set."""
    groups = {}
    for seed in seeds:
        c = case(kernel, seed)
        groups.setdefault(c["set"], []).append(c)
    return sorted(groups.items())


def expect(kernel, s, cases):
    """The probe's result for every case of a batch."""
    row, items = ROWS[kernel], [c["item"] for c in cases]
    if hasattr(row, "expect"):
        return row.expect(row.sets[s], items)
    return row.parse(row.sets[s], items, run_probe(row.probe, row.lines(row.sets[s], items)))


@functools.lru_cache(maxsize=None)
def family(kernel, first=FIRST_SEED, count=FAMILY):
    """[(set index, cases, the probe's results)] of the seeds first .. first + count - 1, computed once."""
    return [(s, cases, expect(kernel, s, cases)) for s, cases in batches(kernel, range(first, first + count))]


def slice_of(got, b):
    cut = lambda v: None if v is None else v[b:b + 1]
    return tuple(cut(v) for v in got) if isinstance(got, tuple) else {k: cut(v) for k, v in got.items()}


def mismatches(kernel, s, cases, want, got):
    """The cases of a batch whose outputs on the GPU differ from the probe's: [(case, message)]."""
    row, items = ROWS[kernel], [c["item"] for c in cases]
    try:
        row.check(got, want, items)
        return []
    except AssertionError:
        pass
    bad = []
    for b, c in enumerate(cases):
        try:
            row.check(slice_of(got, b), want[b:b + 1], items[b:b + 1])
        except AssertionError as e:
            bad.append((c, str(e)[:300]))
    assert bad, "the batch differs, no single case does"
    return bad


def run_batch(ctx, kernel, s, cases, want):
    row = ROWS[kernel]
    return mismatches(kernel, s, cases, want, row.launch(ctx, row.sets[s], [c["item"] for c in cases]))


# ---- CPU: the probe against the restatement, and the conditions on the inputs --------------------------------------------------
def test_the_generator_is_deterministic_and_the_boundaries_come_from_the_headers():
    assert (REFINE_RESIDENT, BA_MAX_KF, BA_MAX_FREE, HYPOTHESES[4]) == (tref.RESIDENT, tba.MAX_KF, tba.MAX_FREE, tpnp.MAX_HYP)
    assert tpose.PIN_STRIDE > POSE_RESIDENT + 1 > WG and WG_RANSAC > WG     # the modules' own pins straddle the same boundaries
    for kernel in KERNELS:
        row = ROWS[kernel]
        assert 4 <= len(row.sets) <= 6 and len(row.edits) >= 10 and row.edits.count("refused") == 1, kernel
        a, b = case(kernel, FIRST_SEED + 3), case(kernel, FIRST_SEED + 3)
        assert row.lines(row.sets[a["set"]], [a["item"]]) == row.lines(row.sets[b["set"]], [b["item"]]), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_probe_equals_the_restatement_on_the_first_cases(kernel):
    """Every output word of the first SAMPLE cases (for the pose graph the first SAMPLE of a few dozen vertices, for the
    two-view RANSAC the first SAMPLE of at most 64 matches: their restatements loop in Python), each restated at its
    place in its batch; the sample holds every edit kind."""
    row = ROWS[kernel]
    keep = row.sample or (lambda item: True)
    seeds, edits, seed = [], set(), FIRST_SEED
    while len(seeds) < SAMPLE or edits != set(row.edits):
        c = case(kernel, seed)
        if keep(c["item"]):
            seeds.append(seed), edits.add(c["edit"])
        seed += 1
        assert seed < FIRST_SEED + 8 * SAMPLE, (kernel, "no sample", sorted(set(row.edits) - edits))
    t0, tied = time.time(), 0
    for s, cases in batches(kernel, seeds):
        want, items = expect(kernel, s, cases), [c["item"] for c in cases]
        for b, c in enumerate(cases):
            row.same(want[b], row.restate(row.sets[s], items, b), tag(c))
            if row.tied is not None:
                tied += bool(row.tied(row.sets[s], items, b))
    print("%s: %d cases restated in %.1f s" % (kernel, len(seeds), time.time() - t0))
    if row.tied is not None:
        print("%s: %d of %d restated cases have two or more hypotheses with the best score" % (kernel, tied, len(seeds)))
        assert tied >= TIED_FLOOR[kernel], (kernel, tied)


# Two or more hypotheses with the best score, measured on the sample of 48 with the restated hypotheses, and half of it as
# the floor: pnp 15, sim3 13, two_view 9.
TIED_FLOOR = dict(pnp=7, sim3=6, two_view=4)

# Measured on the family with the probe alone, and half of it asserted as the floor: the share of the 256 cases that run
# to a normal end (status code 0 after at least one evaluation; a model for the RANSAC kernels; a map point for the
# triangulation), which is also neither below one half nor all of them, and among those the share that stops before the
# maximal evaluation count.
#                                normal  early
MEASURED = dict(pose=(0.598, 0.366),            # 153 of 256, 56 of those
                sim3_refine=(0.566, 0.662),     # 145, 96
                local_ba=(0.582, 0.369),        # 149, 55
                pose_graph=(0.648, 0.331),      # 166, 55
                pnp=(0.742, None),              # 190
                sim3=(0.621, None),             # 159
                two_view=(0.750, None),         # 192
                reconstruct=(0.551, None),      # 141
                triangulate=(0.809, None),      # 207
                covisibility=(0.723, None))     # 185


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_family_meets_the_conditions_on_the_inputs(kernel):
    row = ROWS[kernel]
    codes, normal, early, total = set(), 0, 0, 0
    for s, cases, want in family(kernel):
        seen = {}
        for c, w in zip(cases, want):
            code = row.code(w)
            codes.update(code if isinstance(code, set) else {code})
            total += 1
            if not row.ran(w):
                continue
            normal += 1
            if row.early is not None:
                early += bool(row.early(row.sets[s], w))
            if c["edit"] not in row.twins:
                k = row.key(w)
                assert k not in seen, "identical outputs: %s and %s" % (tag(seen[k]), tag(c))
                seen[k] = c
    print("%s: codes %r, %d of %d run to a normal end (%.3f), %d of those stop early (%.3f)" % (
        kernel, sorted(codes), normal, total, normal / total, early, early / max(normal, 1)))
    assert codes == row.codes, (kernel, sorted(codes))
    assert total == FAMILY and 0.5 <= normal / total < 1.0
    assert normal / total >= MEASURED[kernel][0] / 2
    if row.early is not None:
        assert early / normal >= MEASURED[kernel][1] / 2


# ---- GPU: the library against the probe ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_gpu_family_equals_the_probe(gpu_ctx, kernel):
    """FAMILY cases, one call per parameter set through the module's Device (rubbish-filled padding, sentinel-filled
    outputs, unequal counts); every output word and sentinel against the probe."""
    t0, bad = time.time(), []
    fam = family(kernel)
    t1 = time.time()
    for s, cases, want in fam:
        bad += run_batch(gpu_ctx, kernel, s, cases, want)
    print("%s: %d cases in %d calls, %.1f s for the probe, %.1f s for the library and the comparison" % (
        kernel, sum(len(c) for _, c, _ in fam), len(fam), t1 - t0, time.time() - t1))
    assert not bad, "\n".join("%s: %s" % (tag(c), msg) for c, msg in bad)
