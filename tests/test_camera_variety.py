"""The five batched geometry kernels that take a camera per batch item (pislam_pose_refine_batch, pislam_pnp_ransac_batch,
pislam_sim3_ransac_batch, pislam_sim3_refine_batch, pislam_two_view_reconstruct_batch) at cameras that differ
(DESIGN.md section 5.5).

Their own modules use one camera everywhere: fx = fy = 500, (cx, cy) = (320, 240), the same for both sides of a Sim(3)
pair and for every item of a batch.  A kernel that exchanges fx and fy, cx and cy, cam1 and cam2, or that reads another
item's camera agrees with the restatement bit for bit on such inputs.  Here every item has a camera of its own, CAMS:
three cameras that differ pairwise in every field, with fx / fy on both sides of 1 and off-centre fractional principal
points; a Sim(3) pair has CAMS[k] on side 1 and CAMS[k + 1] on side 2.

Nothing is restated here: the expectations are the per-kernel modules' restatements, their Device classes pack and
launch, their assert_* helpers compare every output word.  Per kernel:
  1. on the CPU, the restatement under every wrong reading of the camera differs from the restatement under the right
     one in a continuous output: a condition on the inputs, which makes the GPU comparison able to fail;
  2. on the CPU, the host probe (the kernel's arithmetic header under the host compiler) against the restatement;
  3. on the GPU, one small batch, a camera per item, fx = 0 and a NaN camera between good items;
  4. on the GPU, a batch larger than the grid whose items cycle through the cameras with period 3 (the grid, 1024, is
     no multiple of 3: item b and item b + grid, which one workgroup handles, have different cameras), with and without
     refused items just before and just after good ones in a workgroup's walk;
  5. on the GPU, accuracy against float64 on scenes under these cameras, with the per-kernel modules' thresholds.
The chains pnp -> pose, sim3 -> pose and sim3 -> sim3 refine pass device buffers on with a camera per item."""
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_pnp_ransac as tpnp
import test_pose_refine as tpose
import test_sim3_ransac as tsim
import test_sim3_refine as tref
import test_two_view_reconstruct as trec
from conftest import ROOT

F32, F64 = np.float32, np.float64

# fx, fy, cx, cy, bf: exact binary32 values.  fx / fy = 1.33, 0.70 and 0.93.
CAMS = np.array([[520, 390, 301.25, 262.5, 47.5],
                 [410, 585, 347.75, 219.375, 33.25],
                 [463.5, 498.25, 322.625, 251.125, 61.75]], F32)
NS = (45, 60, 33)                                # observations per item; the stride is one above the largest
STRIDE = max(NS) + 1
SMALL = [0, 3, 1, 4, 2]                          # the batch of part 3 as indices into a kernel's items: good 0, fx = 0,
GOOD = (0, 2, 4)                                 # good 1, a NaN camera, good 2; GOOD: where the good ones sit in it
HYP, SEED = 48, 5                                # RANSAC hypotheses and seed of part 3
GRID = 1024                                      # part 4: the five launches' cap on the workgroups, WALK_B items on it;
WALK_B, WALK_N, WALK_HYP = GRID + 6, 16, 8       # the RANSAC items are cut to WALK_N observations


def test_the_cameras_differ_in_every_field():
    assert (CAMS.astype(F64).astype(F32) == CAMS).all() and CAMS.dtype == F32
    for a in range(3):
        for b in range(a + 1, 3):
            assert (CAMS[a] != CAMS[b]).all()
    ratio = CAMS[:, 0] / CAMS[:, 1]
    assert ratio.max() > 1.25 and ratio.min() < 0.8
    for c in CAMS:
        assert len(set(c.tolist())) == 5 and c[2] % 1 != 0 and c[3] % 1 != 0
        assert abs(c[2] - 320) > 2 and abs(c[3] - 240) > 2
    assert GRID % 3 != 0


# ---- wrong readings and the count of changed words -----------------------------------------------------------------------
def swap_f(c):
    c = np.array(c, F32)
    c[[0, 1]] = c[[1, 0]]
    return c


def swap_c(c):
    c = np.array(c, F32)
    c[[2, 3]] = c[[3, 2]]
    return c


def no_fx(c):
    c = np.array(c, F32)
    c[0] = 0
    return c


def nan_cy(c):
    c = np.array(c, F32)
    c[3] = np.nan
    return c


def readings(k):
    """The wrong readings of item k's camera: name -> camera."""
    return {"fx <-> fy": swap_f(CAMS[k]), "cx <-> cy": swap_c(CAMS[k]), "the next item's camera": CAMS[(k + 1) % 3],
            "the previous item's camera": CAMS[(k + 2) % 3]}


def pair_readings(k):
    """The wrong readings of a Sim(3) pair's cameras (CAMS[k], CAMS[k + 1]): name -> (cam1, cam2)."""
    c1, c2, c3 = CAMS[k], CAMS[(k + 1) % 3], CAMS[(k + 2) % 3]
    return {"fx1 <-> fy1": (swap_f(c1), c2), "fx2 <-> fy2": (c1, swap_f(c2)), "cx1 <-> cy1": (swap_c(c1), c2),
            "cx2 <-> cy2": (c1, swap_c(c2)), "the next item's cameras": (c2, c3), "the previous item's cameras": (c3, c1),
            "cam1 <-> cam2": (c2, c1), "cam1 for both sides": (c1, c1), "cam2 for both sides": (c2, c2)}


def bits(x):
    a = np.atleast_1d(np.asarray(x))
    return a.view(np.uint64) if a.dtype == F64 else a.view(np.uint32) if a.dtype == F32 else a.astype(np.int64)


def changed(got, want, keys):
    return sum(int((bits(got[k]) != bits(want[k])).sum()) for k in keys)


def discriminates(kernel, item, right, wrong, continuous):
    """wrong: name -> result under that reading.  Prints, per reading, the changed words and asserts that a continuous
    output is among them."""
    for name, r in wrong.items():
        cont, total = changed(r, right, continuous), changed(r, right, list(right))
        print("%-12s %-8s %-28s: %3d words of %s changed, %3d in all" % (kernel, item, name, cont, "/".join(continuous), total))
        assert cont > 0, (kernel, item, name, "this input does not separate the reading: choose another")


# ---- the launch rules ----------------------------------------------------------------------------------------------------
def grid_cap(header, name):
    text = open(os.path.join(ROOT, "pislam_amd", "csrc", header)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


LAUNCH = dict(pose=("pislam_refine_kernels.h", "GRID_CAP", "po::k_pose_refine, dim3((unsigned)std::min(batch, prf::GRID_CAP))"),
              pnp=("pislam_ransac_kernels.h", "GRID_CAP", "pn::k_pnp_ransac, dim3((unsigned)std::min(batch, prk::GRID_CAP))"),
              sim3=("pislam_ransac_kernels.h", "GRID_CAP", "s3::k_sim3_ransac, dim3((unsigned)std::min(batch, prk::GRID_CAP))"),
              refine=("pislam_refine_kernels.h", "GRID_CAP", "sr::k_sim3_refine, dim3((unsigned)std::min(batch, prf::GRID_CAP))"),
              recon=("pislam_recon_kernels.h", "RC_GRID_CAP", "pr::k_reconstruct, dim3((unsigned)std::min(batch, pr::RC_GRID_CAP))"))


def need_a_second_pass(kernel, batch):
    """The condition on the inputs: the launch rule min(batch, cap) gives fewer workgroups than items, and the period of
    the cameras does not divide the grid."""
    grid = min(batch, grid_cap(*LAUNCH[kernel][:2]))
    print("%s: batch %d on a grid of %d workgroups" % (kernel, batch, grid))
    assert batch > grid and grid == GRID, (kernel, batch, grid)


def test_the_launch_rules_are_the_ones_the_walk_tests_use():
    text = open(os.path.join(ROOT, "pislam_amd", "csrc", "pislam_hip.hip")).read()
    for kernel, (_, _, launch) in LAUNCH.items():
        assert launch in text, kernel
        need_a_second_pass(kernel, WALK_B)


def walk_layout(refusals):
    """The index of each of the WALK_B items into [good 0, good 1, good 2, fx = 0, a NaN camera, too few]: b mod 3, and
    with `refusals` the three refused kinds at b = 0, 1, 2 (the same workgroups go on to the good items GRID, GRID + 1,
    GRID + 2) and at GRID + 3, GRID + 4, GRID + 5 (after the good items 3, 4, 5)."""
    which = [b % 3 for b in range(WALK_B)]
    if refusals:
        which[0:3] = [3, 4, 5]
        which[GRID + 3:GRID + 6] = [3, 4, 5]
    for b in range(WALK_B - GRID):                           # one workgroup's consecutive items never share a camera
        assert which[b] >= 3 or which[b + GRID] >= 3 or which[b] != which[b + GRID]
    return which


# ---- the host probes -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """probe(name, lines): the output lines of tools/probes/<name>.cpp, built as the per-kernel modules build it."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    built = {}

    def run(name, lines):
        if name not in built:
            built[name] = str(tmp_path_factory.mktemp(name) / name)
            subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                                   os.path.join(ROOT, "tools", "probes", name + ".cpp"), "-o", built[name]])
        got = subprocess.run([built[name]], input="\n".join(lines) + "\n", check=True, capture_output=True,
                             text=True).stdout.splitlines()
        assert len(got) == len(lines)
        return got
    return run


def same_lines(got, want, lines):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "case %d: %s" % (k, lines[k][:60])


# ==== pislam_pose_refine_batch ============================================================================================
POSE_PRM = tpose.REUSE_PRM


@functools.lru_cache(maxsize=None)
def pose_items():
    """[good 0, good 1, good 2, fx = 0 (not refused by this call: the restatement says what it gives), a NaN camera
    (status 2), too few (status 1)]."""
    good = [tpose.scene(300 + k, n=NS[k], stereo=0.5, outliers=0.1, cam=CAMS[k])[0] for k in range(3)]
    return good + [dict(good[1], cam=no_fx(CAMS[2])), dict(good[1], cam=nan_cy(CAMS[2])), tpose.sub(good[0], 2)]


@functools.lru_cache(maxsize=None)
def pose_want():
    return [tpose.ref_frame(f, POSE_PRM) for f in pose_items()]


# Noise-free scenes under CAMS (n = 200, Q8-rounded observations, no levels), mono, mixed and stereo, with
# test_ref_pose_anchors' thresholds (2e-5 rad, 2e-4), and the module's noisy behaviour scenes under CAMS with
# check_behaviour's.  The seeds are the first ones tried.  The restatement alone, at its worst: noise-free (seeds 1, 2, 3)
# rotation 7.6e-7 rad, translation 5.3e-6; noisy (seeds 1, 2, each mono, mixed and stereo) rotation 0.061 deg,
# translation 0.0090, true inliers kept 99.4 %, outliers accepted 2.5 %.
POSE_EXACT = ((1, 0.0), (2, 0.5), (3, 1.0))
POSE_NOISY = [(seed, stereo) for seed in (1, 2) for stereo in (0.0, 0.5, 1.0)]


@functools.lru_cache(maxsize=None)
def pose_exact_scenes():
    return [tpose.scene(seed, stereo=st, outliers=0.0, noise=0.0, levels=False, cam=CAMS[i])
            for i, (seed, st) in enumerate(POSE_EXACT)]


@functools.lru_cache(maxsize=None)
def pose_noisy_scenes():
    return [tpose.scene(seed, stereo=st, cam=CAMS[i % 3]) for i, (seed, st) in enumerate(POSE_NOISY)]


def check_pose_exact(res):
    for (fr, truth, _), r in zip(pose_exact_scenes(), res):
        rot, tr = tpose.pose_errors(r["pose"], truth)
        print("pose, noise-free under its own camera: rotation %.3g rad, translation %.3g" % (math.radians(rot), tr))
        assert r["status"] & 255 == 0 and r["ninliers"] == 200 and math.radians(rot) < 2e-5 and tr < 2e-4, (rot, tr)


def test_pose_preconditions():
    """Discrimination, and the float64 checks on the restatement alone."""
    for k in range(3):
        fr = pose_items()[k]
        wrong = {name: tpose.ref_frame(dict(fr, cam=c), POSE_PRM) for name, c in readings(k).items()}
        discriminates("pose", "item %d" % k, pose_want()[k], wrong, ("pose", "cost"))
    want = pose_want()
    assert [w["status"] & 255 for w in want] == [0, 0, 0, want[3]["status"] & 255, 2, 1] and want[3]["status"] >> 8 > 0
    check_pose_exact([tpose.ref_frame(s[0]) for s in pose_exact_scenes()])
    tpose.check_behaviour(lambda frames, prm: [tpose.ref_frame(f, prm) for f in frames], scenes=pose_noisy_scenes())


def test_pose_host_probe(probe):
    frames = pose_items() + [s[0] for s in pose_exact_scenes()] + [s[0] for s in pose_noisy_scenes()]
    prms = [POSE_PRM] * len(pose_items()) + [tpose.DEFAULT] * (len(frames) - len(pose_items()))
    want = pose_want() + [tpose.ref_frame(f) for f in frames[len(pose_items()):]]
    lines = [tpose.probe_line(f, p) for f, p in zip(frames, prms)]
    same_lines(probe("pose_host_check", lines), [tpose.result_line(r) for r in want], lines)


def pose_batch(ctx, which, prm=POSE_PRM, what=""):
    frames = [pose_items()[k] for k in which]
    ns = [len(f["obs"]) for f in frames]
    got = tpose.Device(ctx).run(frames, ns, STRIDE, prm)
    tpose.assert_frames(got, [pose_want()[k] for k in which], ns, what)


@pytest.mark.gpu
def test_gpu_pose_a_camera_per_item(gpu_ctx):
    pose_batch(gpu_ctx, SMALL, what="a camera per item")


@pytest.mark.gpu
@pytest.mark.parametrize("refusals", [False, True], ids=["good", "refused_between"])
def test_gpu_pose_item_walk(gpu_ctx, refusals):
    need_a_second_pass("pose", WALK_B)
    pose_batch(gpu_ctx, walk_layout(refusals), what="item walk")


def pose_runner(ctx):
    d = tpose.Device(ctx)

    def run(frames, prm):
        got = d.run(frames, [len(f["obs"]) for f in frames], 200, prm, frames[0].get("level") is not None)
        return [dict(pose=got["pose_out"][b], inlier=got["inlier"][b], ninliers=int(got["ninliers"][b]),
                     cost=float(got["cost"][b]), status=int(got["status"][b])) for b in range(len(frames))]
    return run


@pytest.mark.gpu
def test_gpu_pose_accuracy_under_unequal_cameras(gpu_ctx):
    run = pose_runner(gpu_ctx)
    check_pose_exact(run([s[0] for s in pose_exact_scenes()], tpose.DEFAULT))
    tpose.check_behaviour(run, scenes=pose_noisy_scenes())


# ==== pislam_pnp_ransac_batch ===============================================================================================
PNP_MIN = 10


@functools.lru_cache(maxsize=None)
def pnp_items():
    """[good 0, good 1, good 2, fx = 0 (status 3), a NaN camera (status 3), too few (status 2)], with levels."""
    good = [tpnp.scene(310 + k, n=NS[k], outliers=0.3, levels=True, cam=CAMS[k])[0] for k in range(3)]
    return good + [dict(good[1], cam=no_fx(CAMS[2])), dict(good[1], cam=nan_cy(CAMS[2])), tpnp.sub(good[0], 3)]


def pnp_walk_items():
    it = pnp_items()
    return [tpnp.sub(f, WALK_N) for f in it[:5]] + [it[5]]


@functools.lru_cache(maxsize=None)
def pnp_small_want():
    return [tpnp.ref_frame(pnp_items()[k], b, HYP, SEED, PNP_MIN) for b, k in enumerate(SMALL)]


def pnp_many(frames, hyp, seed, min_inliers):
    """tpnp.ref_frame for every frame of a batch at its batch index, the good frames (one size) stated at once: the
    module's solver and scoring with one element per (frame, hypothesis) and a camera per frame."""
    B = len(frames)
    want = [tpnp.ref_result(f, None, hyp, min_inliers) for f in frames]
    good = [b for b, f in enumerate(frames) if tpnp.cam_ok(f["cam"]) and len(f["obs"]) >= 4]
    n = len(frames[good[0]]["obs"])
    O = [tpnp.ref_obs(frames[b]) for b in good]
    O = {key: np.stack([o[key] for o in O]) for key in O[0]}                              # [G][n]
    draws = np.array([[tpnp.ref_sample(seed, b, k, n) for k in range(hyp)] for b in good])   # [G][hyp][4]
    rows = np.arange(len(good))[:, None]
    cam = np.stack([np.asarray(frames[b]["cam"], F32) for b in good])                    # [G][5]
    valid, T = tpnp.ref_solver(np.repeat(cam, hyp, 0).T.copy(),
                               *({key: v[rows, draws[:, :, j]].reshape(-1) for key, v in O.items()} for j in range(4)))
    G = len(good)
    with np.errstate(all="ignore"):
        inl, add = tpnp.ref_scores([t.reshape(G, hyp, 1) for t in T], cam.T.reshape(5, G, 1, 1),
                                   {key: v[:, None, :] for key, v in O.items()})
    valid = valid.reshape(G, hyp)
    score, T = np.where(valid, add.sum(2), 0), np.stack(T, 1).reshape(G, hyp, 12)
    for i, b in enumerate(good):
        want[b] = tpnp.ref_result(frames[b], dict(valid=valid[i], T=T[i], score=score[i], inl=inl[i]), hyp, min_inliers)
    return want


@functools.lru_cache(maxsize=None)
def pnp_walk_want(refusals):
    items = pnp_walk_items()
    return pnp_many([items[k] for k in walk_layout(refusals)], WALK_HYP, SEED, PNP_MIN)


# The module's behaviour scene (300 observations, 40 % displaced, +-0.75 px, 200 hypotheses) and its noise-free
# variant, under CAMS, seeds 1, 2, 3 (the first ones tried).  The restatement alone: every undisplaced observation an
# inlier (180 of 180 and 300 of 300), no displaced one, |R'R - I| at most 1.6e-6 (the acceptance: 90 %, none, 1e-3).
PNP_SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def pnp_behaviour_scenes():
    noisy = [tpnp.scene(s, cam=CAMS[i]) for i, s in enumerate(PNP_SEEDS)]
    return noisy + [tpnp.scene(s, outliers=0.0, noise=0.0, cam=CAMS[(i + 1) % 3]) for i, s in enumerate(PNP_SEEDS)]


@functools.lru_cache(maxsize=None)
def pnp_behaviour_want():
    return [tpnp.ref_frame(fr, b, 200, 7, 10) for b, (fr, _, _) in enumerate(pnp_behaviour_scenes())]


def check_pnp_behaviour(res):
    """test_behaviour_on_the_host_probe's acceptance."""
    for b, ((fr, truth, good), r) in enumerate(zip(pnp_behaviour_scenes(), res)):
        inl = np.asarray(r["inlier"]).astype(bool)
        R = np.asarray(r["pose"])[:9].astype(F64).reshape(3, 3)
        print("pnp under its own camera, scene %d: %d of %d undisplaced are inliers, %d displaced, |R'R - I| = %.2e" % (
            b, (inl & good).sum(), good.sum(), (inl & ~good).sum(), np.abs(R.T @ R - np.eye(3)).max()))
        assert r["status"] & 255 == 0 and r["best"] >= 0 and r["ninliers"] == inl.sum()
        assert not (inl & ~good).any()
        assert (inl & good).sum() >= 0.9 * good.sum()
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-3


def test_pnp_preconditions():
    for b, k in zip(GOOD, range(3)):
        fr = pnp_items()[k]
        wrong = {name: tpnp.ref_frame(dict(fr, cam=c), b, HYP, SEED, PNP_MIN) for name, c in readings(k).items()}
        discriminates("pnp", "item %d" % k, pnp_small_want()[b], wrong, ("pose",))
    assert [w["status"] & 255 for w in pnp_small_want()] == [0, 3, 0, 3, 0]
    items, want = pnp_walk_items(), pnp_walk_want(True)
    which = walk_layout(True)
    for b in (3, GRID, GRID + 1, GRID + 2):                          # the walk's items, and pnp_many against the module's own
        right = tpnp.ref_frame(items[which[b]], b, WALK_HYP, SEED, PNP_MIN)
        assert tpnp.result_line(right) == tpnp.result_line(want[b]), b
        wrong = {name: tpnp.ref_frame(dict(items[which[b]], cam=c), b, WALK_HYP, SEED, PNP_MIN)
                 for name, c in readings(which[b]).items()}
        discriminates("pnp", "walk %d" % b, right, wrong, ("pose",))
    assert [want[b]["status"] & 255 for b in (0, 1, 2, GRID + 3, GRID + 4, GRID + 5)] == [3, 3, 2, 3, 3, 2]
    assert sum(w["best"] >= 0 for w in pnp_walk_want(False)) > 900
    check_pnp_behaviour(pnp_behaviour_want())


def test_pnp_host_probe(probe):
    lines = [tpnp.probe_line(pnp_items()[k], b, HYP, SEED, PNP_MIN) for b, k in enumerate(SMALL)]
    want = list(pnp_small_want())
    items, which = pnp_walk_items(), walk_layout(True)
    for b in list(range(6)) + list(range(GRID, WALK_B)):
        lines.append(tpnp.probe_line(items[which[b]], b, WALK_HYP, SEED, PNP_MIN))
        want.append(pnp_walk_want(True)[b])
    lines += [tpnp.probe_line(fr, b, 200, 7, 10) for b, (fr, _, _) in enumerate(pnp_behaviour_scenes())]
    want += pnp_behaviour_want()
    same_lines(probe("pnp_host_check", lines), [tpnp.result_line(r) for r in want], lines)


@pytest.mark.gpu
def test_gpu_pnp_a_camera_per_item(gpu_ctx):
    frames = [pnp_items()[k] for k in SMALL]
    ns = [len(f["obs"]) for f in frames]
    got = tpnp.Device(gpu_ctx).run(frames, ns, STRIDE, (HYP, SEED, PNP_MIN))
    tpnp.assert_frames(got, pnp_small_want(), ns, "a camera per item")


@pytest.mark.gpu
@pytest.mark.parametrize("refusals", [False, True], ids=["good", "refused_between"])
def test_gpu_pnp_item_walk(gpu_ctx, refusals):
    need_a_second_pass("pnp", WALK_B)
    items = pnp_walk_items()
    frames = [items[k] for k in walk_layout(refusals)]
    ns = [len(f["obs"]) for f in frames]
    got = tpnp.Device(gpu_ctx).run(frames, ns, WALK_N + 1, (WALK_HYP, SEED, PNP_MIN))
    tpnp.assert_frames(got, pnp_walk_want(refusals), ns, "item walk")


def split_ransac(got, ns, key):
    return [dict(best=int(got["best"][b]), score=int(got["score"][b]), ninliers=int(got["ninliers"][b]),
                 inlier=got["inlier"][b, :n], status=int(got["status"][b]), **{key.replace("_out", ""): got[key][b]})
            for b, n in enumerate(ns)]


@pytest.mark.gpu
def test_gpu_pnp_behaviour_under_unequal_cameras(gpu_ctx):
    frames = [s[0] for s in pnp_behaviour_scenes()]
    got = tpnp.Device(gpu_ctx).run(frames, [300] * len(frames), 300, (200, 7, 10), False)
    tpnp.assert_frames(got, pnp_behaviour_want(), [300] * len(frames), "behaviour")
    check_pnp_behaviour(split_ransac(got, [300] * len(frames), "pose_out"))


@pytest.mark.gpu
def test_gpu_pnp_chain_into_pose_refine_with_a_camera_per_item(gpu_ctx):
    """test_pnp_chain_into_pose_refine with a camera per frame: the refined mask holds no displaced observation and
    equals the mask the pose call reaches from the ground-truth pose."""
    from pislam_amd.frontend import pnpRansacBatch, poseRefineBatch
    d = tpnp.Device(gpu_ctx)
    scenes = pnp_behaviour_scenes()[:3]
    dev = d.upload(d.pack([s[0] for s in scenes], [300] * 3, 300, False))
    best, score, ninl, inl, pose, status = pnpRansacBatch(dev["cam"], dev["xw"], dev["obs"], dev["counts"], hypotheses=200,
                                                          seed=7, ctx=gpu_ctx)
    truth = d.up(np.stack([np.concatenate([R.reshape(-1), tt]) for _, (R, tt), _ in scenes]).astype(F32))
    out = poseRefineBatch(pose, dev["cam"], dev["xw"], dev["obs"], dev["counts"], ctx=gpu_ctx)
    ref = poseRefineBatch(truth, dev["cam"], dev["xw"], dev["obs"], dev["counts"], ctx=gpu_ctx)
    gpu_ctx.synchronize()
    assert (status.cpu().numpy() & 255 == 0).all()
    assert (out[4].cpu().numpy() & 255 == 0).all() and (ref[4].cpu().numpy() & 255 == 0).all()
    m, mr = out[1].cpu().numpy().astype(bool), ref[1].cpu().numpy().astype(bool)
    for b, (_, _, good) in enumerate(scenes):
        assert not (m[b] & ~good).any() and m[b].sum() >= 0.9 * good.sum()
        assert (m[b] == mr[b]).all(), b


# ==== pislam_sim3_ransac_batch ==============================================================================================
SIM3_MIN = 10


def pair_scene(seed, k, **kw):
    return tsim.scene(seed, cam1=CAMS[k % 3], cam2=CAMS[(k + 1) % 3], **kw)


def with_cams(pr, cam1, cam2):
    return dict(pr, cam1=np.array(cam1, F32), cam2=np.array(cam2, F32))


@functools.lru_cache(maxsize=None)
def sim3_items():
    """[good 0, good 1, good 2, fx1 = 0 (status 3), a NaN camera 2 (status 3), too few (status 2)]: levels on both sides
    (the two sides' level arrays differ), cam1 = CAMS[k], cam2 = CAMS[k + 1]."""
    good = [pair_scene(320 + k, k, n=NS[k], outliers=0.3, levels=True)[0] for k in range(3)]
    return good + [with_cams(good[1], no_fx(CAMS[2]), CAMS[0]), with_cams(good[1], CAMS[2], nan_cy(CAMS[0])), tsim.sub(good[0], 2)]


def sim3_walk_items():
    it = sim3_items()
    return [tsim.sub(p, WALK_N) for p in it[:5]] + [it[5]]


@functools.lru_cache(maxsize=None)
def sim3_small_want(fixed=False):
    return [tsim.ref_pair(sim3_items()[k], b, HYP, SEED, SIM3_MIN, fixed) for b, k in enumerate(SMALL)]


@functools.lru_cache(maxsize=None)
def sim3_walk_want(refusals):
    items = sim3_walk_items()
    pairs = [items[k] for k in walk_layout(refusals)]
    want = [tsim.ref_result(p, None, WALK_HYP, SIM3_MIN) for p in pairs]
    good = [b for b, p in enumerate(pairs) if tsim.cam_ok(p["cam1"]) and tsim.cam_ok(p["cam2"]) and len(p["obs1"]) >= 3]
    all_ = tsim.ref_batch([pairs[b] for b in good], good, SEED, WALK_HYP, False)
    for i, b in enumerate(good):
        want[b] = tsim.ref_result(pairs[b], {k: v[i] for k, v in all_.items()}, WALK_HYP, SIM3_MIN)
    return want


# The module's behaviour scene (n = 300, 40 % replaced, 0.75 px, 1 % depth noise, 200 hypotheses, RANSAC seed 7) and its
# noise-free variant under unequal cameras, scene seeds 1, 2, 3 (the first ones tried): float64 Horn RANSAC alone and
# the restatement meet the module's caps (70 % kept, 2 % of the replaced) on all six.  The restatement keeps 172, 171
# and 163 of 180 on the noisy scenes and all 180 on the noise-free ones, none of the replaced; |R'R - I| <= 5.6e-7.
SIM3_SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def sim3_behaviour_scenes():
    noisy = [pair_scene(s, i) for i, s in enumerate(SIM3_SEEDS)]
    return noisy + [pair_scene(s, i + 1, noise=0.0, depth_noise=0.0) for i, s in enumerate(SIM3_SEEDS)]


@functools.lru_cache(maxsize=None)
def sim3_behaviour_want():
    return [tsim.ref_pair(pr, b, 200, tsim.BEHAVIOUR_SEED) for b, (pr, _, _) in enumerate(sim3_behaviour_scenes())]


def check_sim3_behaviour(res):
    for b, ((pr, (R, t, sc), good), r) in enumerate(zip(sim3_behaviour_scenes(), res)):
        inl = np.asarray(r["inlier"]).astype(bool)
        Re = np.asarray(r["sim"])[:9].astype(F64).reshape(3, 3)
        print("sim3 under unequal cameras, scene %d: %d of %d kept, %d replaced, |R'R - I| = %.2e, s %.4f (true %.4f)" % (
            b, (inl & good).sum(), good.sum(), (inl & ~good).sum(), np.abs(Re.T @ Re - np.eye(3)).max(), r["sim"][12], sc))
        assert r["status"] & 255 == 0 and r["best"] >= 0 and r["ninliers"] == inl.sum()
        tsim.assert_caps(inl, good, 0.70, "scene %d" % b)
        assert np.abs(Re.T @ Re - np.eye(3)).max() < 1e-5


def test_sim3_preconditions():
    for b, k in zip(GOOD, range(3)):
        pr = sim3_items()[k]
        wrong = {name: tsim.ref_pair(with_cams(pr, *c), b, HYP, SEED, SIM3_MIN) for name, c in pair_readings(k).items()}
        discriminates("sim3", "item %d" % k, sim3_small_want()[b], wrong, ("sim", "score"))
    assert [w["status"] & 255 for w in sim3_small_want()] == [0, 3, 0, 3, 0]
    items, want, which = sim3_walk_items(), sim3_walk_want(True), walk_layout(True)
    for b in (3, GRID, GRID + 1, GRID + 2):
        right = tsim.ref_pair(items[which[b]], b, WALK_HYP, SEED, SIM3_MIN)
        assert tsim.result_line(right) == tsim.result_line(want[b]), b
        wrong = {name: tsim.ref_pair(with_cams(items[which[b]], *c), b, WALK_HYP, SEED, SIM3_MIN)
                 for name, c in pair_readings(which[b]).items()}
        discriminates("sim3", "walk %d" % b, right, wrong, ("sim", "score"))
    assert [want[b]["status"] & 255 for b in (0, 1, 2, GRID + 3, GRID + 4, GRID + 5)] == [3, 3, 2, 3, 3, 2]
    assert sum(w["best"] >= 0 for w in sim3_walk_want(False)) > 900
    for b, (pr, _, good) in enumerate(sim3_behaviour_scenes()):
        tsim.assert_caps(tsim.ransac64(pr, b, 200, tsim.BEHAVIOUR_SEED), good, 0.70, "float64, scene %d" % b)
    check_sim3_behaviour(sim3_behaviour_want())


def test_sim3_host_probe(probe):
    lines, want = [], []
    for fixed in (False, True):
        lines += [tsim.probe_line(sim3_items()[k], b, HYP, SEED, SIM3_MIN, fixed) for b, k in enumerate(SMALL)]
        want += sim3_small_want(fixed)
    items, which = sim3_walk_items(), walk_layout(True)
    for b in list(range(6)) + list(range(GRID, WALK_B)):
        lines.append(tsim.probe_line(items[which[b]], b, WALK_HYP, SEED, SIM3_MIN, False))
        want.append(sim3_walk_want(True)[b])
    lines += [tsim.probe_line(pr, b, 200, tsim.BEHAVIOUR_SEED, 20, False) for b, (pr, _, _) in enumerate(sim3_behaviour_scenes())]
    want += sim3_behaviour_want()
    same_lines(probe("sim3_host_check", lines), [tsim.result_line(r) for r in want], lines)


@pytest.mark.gpu
@pytest.mark.parametrize("fixed", [False, True], ids=["free_scale", "fixed_scale"])
def test_gpu_sim3_a_camera_per_side_and_item(gpu_ctx, fixed):
    pairs = [sim3_items()[k] for k in SMALL]
    ns = [len(p["obs1"]) for p in pairs]
    got = tsim.Device(gpu_ctx).run(pairs, ns, STRIDE, (HYP, SEED, SIM3_MIN, int(fixed)))
    tsim.assert_pairs(got, sim3_small_want(fixed), ns, "a camera per side and item")


@pytest.mark.gpu
@pytest.mark.parametrize("refusals", [False, True], ids=["good", "refused_between"])
def test_gpu_sim3_item_walk(gpu_ctx, refusals):
    need_a_second_pass("sim3", WALK_B)
    items = sim3_walk_items()
    pairs = [items[k] for k in walk_layout(refusals)]
    ns = [len(p["obs1"]) for p in pairs]
    got = tsim.Device(gpu_ctx).run(pairs, ns, WALK_N + 1, (WALK_HYP, SEED, SIM3_MIN, 0))
    tsim.assert_pairs(got, sim3_walk_want(refusals), ns, "item walk")


@pytest.mark.gpu
def test_gpu_sim3_behaviour_under_unequal_cameras(gpu_ctx):
    pairs = [s[0] for s in sim3_behaviour_scenes()]
    got = tsim.Device(gpu_ctx).run(pairs, [300] * len(pairs), 300, (200, tsim.BEHAVIOUR_SEED, 20, 0), False)
    tsim.assert_pairs(got, sim3_behaviour_want(), [300] * len(pairs), "behaviour")
    check_sim3_behaviour(split_ransac(got, [300] * len(pairs), "sim_out"))


@pytest.mark.gpu
def test_gpu_sim3_chain_into_pose_refine_with_unequal_cameras(gpu_ctx):
    """test_sim3_chain_into_pose_refine with cam1 != cam2 and other cameras per pair: the pose call runs under cam1."""
    from pislam_amd.frontend import poseRefineBatch, sim3RansacBatch
    d = tsim.Device(gpu_ctx)
    scenes = [pair_scene(s, i, depth_noise=0.0, fixed_scale=True) for i, s in enumerate(tsim.CHAIN_SEEDS)]
    dev = d.upload(d.pack([s[0] for s in scenes], [300] * 3, 300, False))
    best, score, ninl, inl, sim, status = sim3RansacBatch(*(dev[k] for k in tsim.IN_NAMES), hypotheses=200, seed=7,
                                                          fixed_scale=True, ctx=gpu_ctx)
    pose = sim[:, :12].contiguous()
    truth = d.up(np.stack([np.concatenate([R.reshape(-1), tt]) for _, (R, tt, _), _ in scenes]).astype(F32))
    out = poseRefineBatch(pose, dev["cam1"], dev["x2"], dev["obs1"], dev["counts"], ctx=gpu_ctx)
    ref = poseRefineBatch(truth, dev["cam1"], dev["x2"], dev["obs1"], dev["counts"], ctx=gpu_ctx)
    gpu_ctx.synchronize()
    assert (status.cpu().numpy() & 255 == 0).all() and (sim[:, 12].cpu().numpy() == 1.0).all()
    assert (out[4].cpu().numpy() & 255 == 0).all() and (ref[4].cpu().numpy() & 255 == 0).all()
    m, mr = out[1].cpu().numpy().astype(bool), ref[1].cpu().numpy().astype(bool)
    po, pr_ = out[0].cpu().numpy().astype(F64), ref[0].cpu().numpy().astype(F64)
    for b, (_, (R, tt, _), good) in enumerate(scenes):
        assert not (m[b] & ~good).any() and m[b].sum() >= 0.9 * good.sum()
        assert (m[b] == mr[b]).all(), b
        assert np.abs(po[b, :9] - pr_[b, :9]).max() < 1e-3 and np.abs(po[b, 9:] - pr_[b, 9:]).max() < 1e-2, b
        assert np.abs(po[b, :9] - R.reshape(-1)).max() < 1e-2 and np.abs(po[b, 9:] - tt).max() < 1e-1, b


# ==== pislam_sim3_refine_batch ==============================================================================================
REFINE_PRM = tref.REUSE_PRM


@functools.lru_cache(maxsize=None)
def refine_items():
    """(pair, sim_in, mask) of [good 0, good 1 (with a mask), good 2, fy2 = 0 (status 2), a NaN camera 1 (status 2), too
    few (status 1)]."""
    out = []
    for k in range(3):
        pr, truth, _ = pair_scene(340 + k, k, n=NS[k], outliers=0.2, levels=True)
        out.append((pr, tref.truth_sim(truth, 0.01, 0.05, 0.02, seed=k), tref.with_mask(NS[k], k) if k == 1 else None))
    no_fy = np.array(CAMS[0], F32)
    no_fy[1] = 0
    pr, sim, _ = out[1]
    return out + [(with_cams(pr, CAMS[2], no_fy), sim, None), (with_cams(pr, nan_cy(CAMS[2]), CAMS[0]), sim, None),
                  (tsim.sub(out[0][0], 2), out[0][1], None)]


@functools.lru_cache(maxsize=None)
def refine_want(prm=REFINE_PRM):
    return [tref.ref_refine(pr, sim, prm, mask) for pr, sim, mask in refine_items()]


# Noise-free scenes under unequal cameras (n = 200, started 0.05 rad, 0.2 and 10 % off), tref.EXACT_PRM, scene seeds
# 1, 2, 3 (the first ones tried), free and fixed scale.  The restatement's worst errors over the six runs: rotation
# 3.76e-5 deg, translation 2.89e-6, |log(s / s_true)| 3.9e-7, inside the module's bounds (9.45e-5, 8.43e-6, 5.13e-6),
# which stay as they are.
REFINE_SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def refine_exact_scenes():
    out = []
    for fixed in (False, True):
        for i, seed in enumerate(REFINE_SEEDS):
            pr, truth, _ = pair_scene(seed, i + int(fixed), n=200, outliers=0.0, noise=0.0, depth_noise=0.0, fixed_scale=fixed)
            out.append((pr, truth, tref.truth_sim(truth, 0.05, 0.2, 0.0 if fixed else 0.1, seed=seed),
                        tref.with_fixed(tref.EXACT_PRM, fixed)))
    return out


@functools.lru_cache(maxsize=None)
def refine_exact_want():
    return [tref.ref_refine(pr, start, prm) for pr, _, start, prm in refine_exact_scenes()]


REFINE_EXACT_BOUND = tref.EXACT_BOUND


def check_refine_exact(res):
    """check_accuracy's noise-free half: the float64 reference converges onto the truth, the call ends within
    REFINE_EXACT_BOUND of the truth."""
    worst = dict(rot=0.0, tr=0.0, sc=0.0)
    for (pr, truth, start, prm), r in zip(refine_exact_scenes(), res):
        assert r["status"] & 255 == 0 and r["ninliers"] == 200
        for k, v in zip(("rot", "tr", "sc"), tref.sim_errors(r["sim"], truth)):
            worst[k] = max(worst[k], v)
    print("sim3 refine under unequal cameras, noise-free, worst errors: %r (bounds %r)" % (worst, REFINE_EXACT_BOUND))
    for k, v in worst.items():
        assert v <= REFINE_EXACT_BOUND[k], (k, v)


def test_refine_preconditions():
    for k in range(3):
        pr, sim, mask = refine_items()[k]
        wrong = {name: tref.ref_refine(with_cams(pr, *c), sim, REFINE_PRM, mask) for name, c in pair_readings(k).items()}
        discriminates("sim3 refine", "item %d" % k, refine_want()[k], wrong, ("sim", "cost"))
    assert [w["status"] & 255 for w in refine_want()] == [0, 0, 0, 2, 2, 1]
    for pr, truth, start, prm in refine_exact_scenes():
        ref = tref.lm64(pr, start, prm)
        assert ref["conv"] and ref["inlier"].all()
        miss = max(a / b for a, b in zip(tref.sim_errors(ref["sim"], truth), (1e-4, 1e-5, 1e-5)))
        assert miss < 1, "the reference misses the truth"
    check_refine_exact(refine_exact_want())


def test_refine_host_probe(probe):
    lines = [tref.probe_line(pr, sim, REFINE_PRM, mask) for pr, sim, mask in refine_items()]
    want = list(refine_want())
    fixed = tref.with_fixed(REFINE_PRM, True)
    lines += [tref.probe_line(pr, sim, fixed, mask) for pr, sim, mask in refine_items()]
    want += refine_want(fixed)
    lines += [tref.probe_line(pr, start, prm) for pr, _, start, prm in refine_exact_scenes()]
    want += refine_exact_want()
    same_lines(probe("sim3_refine_host_check", lines), [tref.result_line(r) for r in want], lines)


def refine_batch(ctx, which, prm=REFINE_PRM, what=""):
    trip = [refine_items()[k] for k in which]
    ns = [len(t[0]["obs1"]) for t in trip]
    got = tref.Device(ctx).run(trip, ns, STRIDE, prm)
    tref.assert_pairs(got, [refine_want(prm)[k] for k in which], ns, what)


@pytest.mark.gpu
@pytest.mark.parametrize("fixed", [False, True], ids=["free_scale", "fixed_scale"])
def test_gpu_refine_a_camera_per_side_and_item(gpu_ctx, fixed):
    refine_batch(gpu_ctx, SMALL, tref.with_fixed(REFINE_PRM, fixed), "a camera per side and item")


@pytest.mark.gpu
@pytest.mark.parametrize("refusals", [False, True], ids=["good", "refused_between"])
def test_gpu_refine_item_walk(gpu_ctx, refusals):
    need_a_second_pass("refine", WALK_B)
    refine_batch(gpu_ctx, walk_layout(refusals), what="item walk")


@pytest.mark.gpu
def test_gpu_refine_accuracy_under_unequal_cameras(gpu_ctx):
    scenes = refine_exact_scenes()
    d, res = tref.Device(gpu_ctx), []
    for k in (0, 3):                                         # one call per parameter set: free, then fixed scale
        part = scenes[k:k + 3]
        got = d.run([(pr, start, None) for pr, _, start, _ in part], [200] * 3, 200, part[0][3], False)
        tref.assert_pairs(got, refine_exact_want()[k:k + 3], [200] * 3, "noise-free")
        res += tref.split(got, [200] * 3)
    check_refine_exact(res)


@pytest.mark.gpu
def test_gpu_refine_chain_from_the_ransac_call_with_unequal_cameras(gpu_ctx):
    """test_sim3_refine_chain_from_the_ransac_call with cam1 != cam2 and other cameras per pair: every output word
    equals the restatement of the chain, free and fixed scale."""
    from pislam_amd.frontend import sim3RansacBatch, sim3RefineBatch
    d = tref.Device(gpu_ctx)
    for fixed in (False, True):
        scenes = [pair_scene(s, i, n=300 - 40 * i, levels=True, fixed_scale=fixed)[0] for i, s in enumerate(tref.CHAIN_SEEDS)]
        ns = [len(pr["obs1"]) for pr in scenes]
        h = d.pack([(pr, tref.IDENTITY, None) for pr in scenes], ns, 300)
        dev = d.upload(h)
        kw = dict(level1=dev["level1"], level2=dev["level2"], inv_sigma2=h["tab"], fixed_scale=fixed, ctx=gpu_ctx)
        ins = tuple(dev[k] for k in tref.IN_NAMES[1:])
        _, _, _, inl, sim, status = sim3RansacBatch(*ins, hypotheses=64, seed=7, **kw)
        out = sim3RefineBatch(sim, *ins, mask=inl, **kw, **d.sentinels(3, 300))
        gpu_ctx.synchronize()
        got = dict(zip(tref.OUT_NAMES, (x.cpu().numpy() for x in out)))
        want = []
        for b, pr in enumerate(scenes):
            ra = tsim.ref_pair(pr, b, 64, 7, 20, fixed)
            assert ra["status"] & 255 == 0 and int(status[b]) == ra["status"]
            want.append(tref.ref_refine(pr, ra["sim"], tref.with_fixed(tref.DEFAULT, fixed), ra["inlier"]))
            assert want[-1]["status"] & 255 == 0 and want[-1]["ninliers"] >= 0.4 * ns[b]
        tref.assert_pairs(got, want, ns, "chain, fixed %d" % fixed)


# ==== pislam_two_view_reconstruct_batch =====================================================================================
RECON_PRM = (256, trec.COS_1DEG, F32(0.99998), 5, 90, 70, 6)


@functools.lru_cache(maxsize=None)
def recon_items():
    """dict(q1, q2, cam, cand) of [good 0, good 1, good 2, fx = 0 (code 4), a NaN camera (code 4), too few (code 1)]:
    four candidates with the truth at place k."""
    good = []
    for k in range(3):
        sc = trec.scene(330 + k, NS[k], far=5, cam=CAMS[k, :4])
        good.append(dict(q1=sc["q1"], q2=sc["q2"], cam=CAMS[k, :4].copy(), cand=trec.eight_motions(sc, k, first=k)[:4]))
    few = {k: (v[:2] if k in ("q1", "q2") else v) for k, v in good[0].items()}
    return good + [dict(good[1], cam=no_fx(CAMS[2, :4])), dict(good[1], cam=nan_cy(CAMS[2, :4])), few]


def recon_pack(items, stride):
    """(q1, q2, counts, cam, cand) of a batch; the slots at and beyond a pair's matches hold rubbish."""
    B = len(items)
    rng = np.random.default_rng(17)
    q1, q2 = (rng.integers(-1 << 31, 1 << 31, (B, stride, 2)) for _ in range(2))
    for b, it in enumerate(items):
        n = len(it["q1"])
        q1[b, :n], q2[b, :n] = it["q1"], it["q2"]
    return (q1, q2, np.array([len(it["q1"]) for it in items], np.uint32), np.stack([it["cam"] for it in items]).astype(F32),
            np.stack([it["cand"] for it in items]).astype(F32))


def recon_one(item):
    r = trec.ref_batch(*recon_pack([item], max(1, len(item["q1"])))[:3], None, item["cam"][None], item["cand"][None], RECON_PRM)
    return {k: v[0] for k, v in r.items()}


def recon_batch_want(which, stride):
    q1, q2, counts, cam, cand = recon_pack([recon_items()[k] for k in which], stride)
    return (q1, q2, counts, cam, cand), trec.ref_batch(q1, q2, counts, None, cam, cand, RECON_PRM)


RECON_B = 12


@functools.lru_cache(maxsize=None)
def recon_sequence():
    """sequence_scene()'s layout with a camera per pair: 12 pairs of 600 points, the candidates twoViewCandidates' of
    the true F under the pair's own K.  The restatement's largest relative depth error on it is 1.44e-4 (check_sequence's
    bound, derived for f = 500, is 1e-3: at the smallest focal length here, 390, one image's share is 8e-5, not 7e-5)."""
    from pislam_amd.frontend import twoViewCandidates
    scs = [trec.scene(900 + b, trec.SEQ_N, cam=CAMS[b % 3, :4]) for b in range(RECON_B)]
    cand = []
    for b, sc in enumerate(scs):
        fx, fy, cx, cy = (float(c) for c in CAMS[b % 3, :4])
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
        Ki, t = np.linalg.inv(K), sc["t"]
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        cand.append(twoViewCandidates("F", Ki.T @ tx @ sc["R"] @ Ki, K))
    cand = np.stack(cand)
    assert cand.shape == (RECON_B, 4, 12) and cand.dtype == F32 and np.isfinite(cand).all()
    truth = []
    for b, sc in enumerate(scs):
        hit = [c for c in range(4) if np.abs(cand[b, c] - trec.motion(sc["R"], sc["t"] / np.linalg.norm(sc["t"]))).max() < 1e-6]
        assert len(hit) == 1
        truth.append(hit[0])
    return dict(q1=np.stack([s["q1"] for s in scs]), q2=np.stack([s["q2"] for s in scs]), cand=cand,
                cam=np.stack([CAMS[b % 3, :4] for b in range(RECON_B)]), truth=np.array(truth),
                z=np.stack([s["X1"][:, 2] for s in scs]))


@functools.lru_cache(maxsize=None)
def recon_sequence_want():
    s = recon_sequence()
    return trec.ref_batch(s["q1"], s["q2"], [trec.SEQ_N] * RECON_B, None, s["cam"], s["cand"], trec.DEFAULT)


def test_recon_preconditions():
    for k in range(3):
        it = recon_items()[k]
        right = recon_one(it)
        assert right["status"] == k << 8 and right["best"] == k and right["point"].sum() >= NS[k] - 8
        wrong = {name: recon_one(dict(it, cam=c[:4])) for name, c in readings(k).items()}
        discriminates("reconstruct", "item %d" % k, right, wrong, ("xw", "pose_out"))
    assert [int(recon_one(it)["status"]) & 255 for it in recon_items()[3:]] == [4, 4, 1]
    r = recon_sequence_want()
    trec.check_sequence(r["best"], r["status"], r["xw"], r["point"], recon_sequence())


def test_recon_host_probe(probe):
    (q1, q2, counts, cam, cand), r = recon_batch_want(range(6), STRIDE)
    lines = [trec.probe_line(q1[b], q2[b], int(r["n"][b]), None, cam[b], cand[b], RECON_PRM) for b in range(6)]
    want = [trec.result_line(r, b) for b in range(6)]
    s, rs = recon_sequence(), recon_sequence_want()
    for b in range(3):
        lines.append(trec.probe_line(s["q1"][b], s["q2"][b], trec.SEQ_N, None, s["cam"][b], s["cand"][b], trec.DEFAULT))
        want.append(trec.result_line(rs, b))
    same_lines(probe("recon_host_check", lines), want, lines)


@pytest.mark.gpu
def test_gpu_recon_a_camera_per_item(gpu_ctx):
    (q1, q2, counts, cam, cand), want = recon_batch_want(SMALL, STRIDE)
    assert (want["status"] & 255).tolist() == [0, 4, 0, 4, 0]
    trec.assert_same(trec.Device(gpu_ctx).run(q1, q2, counts, None, cam, cand, RECON_PRM), want, "a camera per item")


@pytest.mark.gpu
@pytest.mark.parametrize("refusals", [False, True], ids=["good", "refused_between"])
def test_gpu_recon_item_walk(gpu_ctx, refusals):
    need_a_second_pass("recon", WALK_B)
    which = walk_layout(refusals)
    (q1, q2, counts, cam, cand), want = recon_batch_want(which, STRIDE)
    assert (want["best"] == np.where(np.array(which) < 3, which, -1)).all()
    trec.assert_same(trec.Device(gpu_ctx).run(q1, q2, counts, None, cam, cand, RECON_PRM), want, "item walk")


@pytest.mark.gpu
def test_gpu_recon_sequence_with_a_camera_per_pair(gpu_ctx):
    s = recon_sequence()
    got = trec.Device(gpu_ctx).run(s["q1"], s["q2"], [trec.SEQ_N] * RECON_B, None, s["cam"], s["cand"], trec.DEFAULT)
    trec.assert_same(got, recon_sequence_want(), "sequence")
    trec.check_sequence(got["best"], got["status"], got["xw"], got["point"], s)
