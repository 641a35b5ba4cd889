"""CPU suite: what the back-end wrappers of pislam_amd/frontend.py hand to the C ABI, and what they refuse, held fixed.

The wrappers (WRAPPERS below: orbAnglesBatch ... bowWeightBatch, and the four matchers that share their output allocation
with matchEpipolarBatch) compute nothing; they check their tensors, marshal host tables
and parameter structs, allocate missing outputs and call one library function.  Here each runs on CPU tensors with a recording
stand-in for the context: its `lib.<anything>(*args)` appends the call and returns 0, its `check` notes the name it was given.
No library is loaded and no device is touched.

Good calls are recorded as what reaches the library, argument by argument:
  "ctx"            the context handle
  "<name>"         the address of the tensor the test passed as argument <name> (an output passed in, or an in-place form)
  "new:<i>"        the address of a tensor the wrapper allocated: the i-th entry of what it returns
  "null"           None or 0 (a null pointer, or the table length without a table)
  hex string       the bytes of the parameter struct passed by reference
  [hex words]      the 32-bit words of a C float array (a level table)
  integer          itself
and, per returned entry, null or its dtype, its shape and which argument it is ("is": null for a new tensor).  Refused calls
are recorded as the exact ValueError message; none of them may reach the stand-in.  The single-fault refusals and the
"first+last" ones (the first and the last checked argument both bad) together pin the order of the checks.

tests/golden/backend_wrapper_calls.json holds the record, as the wrappers answered before their checks and table marshalling
were stated once (the commit is named in the file).  `python tests/test_backend_wrappers.py` re-records it from the
pislam_amd/frontend.py in the tree, and while the wrappers still raise their messages themselves it also checks, from the source,
that every `raise ValueError` of every wrapper is reached.  Re-recording is right for a change that is meant to alter what a
wrapper passes or refuses; a change that is meant to keep the wrappers' behaviour (a refactor of the checks, a new helper)
keeps this file as it is and must pass against it.

The one path no CPU test reaches, numpy inputs (they go to the device), is the GPU test at the end."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from pislam_amd import frontend as fe

RECORD = os.path.join(GOLDEN, "backend_wrapper_calls.json")

# distinct extents, so that a swapped stride shows: batch, stride (q_stride), t_stride, key frames, points, vertices, edges
B, S, TS, KF, PT, V, E = 2, 8, 7, 3, 5, 4, 6
F32, F64, I16, I32, I64, U8 = torch.float32, torch.float64, torch.int16, torch.int32, torch.int64, torch.uint8
U16, U32 = torch.uint16, torch.uint32


class Recorder:
    """The stand-in for a Context: nothing behind it."""

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


def z(dtype, *shape):
    return torch.zeros(shape, dtype=dtype)


def strided(t):
    """t's dtype and shape, but every other element of a buffer twice as long: not contiguous."""
    return torch.zeros(tuple(t.shape[:-1]) + (2 * int(t.shape[-1]),), dtype=t.dtype)[..., ::2]


# ---- how a case changes the good call it starts from: functions of the call so far, returning the arguments to replace
def put(**kw):
    return lambda b: {k: (v() if callable(v) else v) for k, v in kw.items()}


def retype(name, dtype):
    return lambda b: {name: b[name].to(dtype)}


def reshape(name, *shape):
    return lambda b: {name: z(b[name].dtype, *shape)}


def stride_of(name):
    return lambda b: {name: strided(b[name])}


def both(*steps):
    def change(b):
        out = {}
        for s in steps:
            out.update(s({**b, **out}))
        return out
    return change


def refusals(names, wrong):
    """{case: change} for the usual faults of tensors: wrong = {name: (a dtype it must not have or None, a shape it must not
    have)}; `names` are those swept for contiguity."""
    out = {}
    for n, (dt, shape) in wrong.items():
        if dt is not None:
            out[f"{n}-dtype"] = retype(n, dt)
        if shape is not None:
            out[f"{n}-shape"] = reshape(n, *shape)
    for n in names:
        out[f"{n}-strided"] = stride_of(n)
    return out


def with_first(first, cases):
    """Each case on top of `first` (an optional input that has to be present for the fault to be looked at)."""
    return {k: both(first, c) for k, c in cases.items()}


# ---- the wrappers: a good call with defaults, good variants, refused variants ---------------------------------------------
W = {}

# the four matchers that allocate (idx, dist, dist2) as matchEpipolarBatch does
_pair = lambda: dict(qdesc=z(I32, B, S, 8), qcounts=z(I32, B), tdesc=z(I32, B, TS, 8), tcounts=z(I32, B))
_kp_pair = lambda: dict(qkp=z(I32, B, S), tkp=z(I32, B, TS), **_pair())
_idx_given = put(idx=lambda: z(I32, B, S), dist=lambda: z(I32, B, S), dist2=lambda: z(I32, B, S))
_two_levels = [(64, 48, 0), (53, 40, 48, 3)]

W["matchHammingBatch"] = dict(base=_pair, good={"defaults": put(), "outputs-given": _idx_given}, refused={})

W["matchHammingWindowBatch"] = dict(
    base=lambda: dict(_kp_pair(), levels=_two_levels, radius=5),
    good={"defaults": put(), "radius-per-level": put(radius=[5, 7]), "outputs-given": _idx_given},
    refused={"tdesc-words": reshape("tdesc", B, TS, 4), "radius-count": put(radius=[5, 7, 9]),
             "first+last": both(reshape("tdesc", B, TS, 4), put(radius=[5, 7, 9]))})

W["matchHammingScaledWindowBatch"] = dict(
    base=lambda: dict(_kp_pair(), levels=_two_levels, scale_q16=None, radius0=5),
    good={"defaults": put(), "scales-given": put(scale_q16=[65536, 79000], radius0=[5, 7]), "one-scale": put(scale_q16=70000),
          "prediction-and-span": put(qpred=lambda: z(I32, B, S, 2), level_span=2), "outputs-given": _idx_given},
    refused={"tdesc-words": reshape("tdesc", B, TS, 4),
             "qpred-dtype": put(qpred=lambda: z(I64, B, S, 2)), "qpred-shape": put(qpred=lambda: z(I32, B, S + 1, 2)),
             "radius0-count": put(radius0=[5, 7, 9]), "scale_q16-count": put(scale_q16=[65536, 79000, 90000]),
             "first+last": both(reshape("tdesc", B, TS, 4), put(scale_q16=[65536, 79000, 90000]))})

W["matchHammingBowBatch"] = dict(
    base=lambda: dict(qdesc=z(I32, B, S, 8), qgroup=z(I32, B, S), qcounts=z(I32, B), tdesc=z(I32, B, TS, 8), tgroup=z(I32, B, TS),
                      tcounts=z(I32, B), ngroups=10),
    good={"defaults": put(), "parameters": put(ngroups=33), "outputs-given": _idx_given},
    refused={"tdesc-words": reshape("tdesc", B, TS, 4), "qgroup-shape": reshape("qgroup", B, S + 1),
             "tgroup-shape": reshape("tgroup", B, TS + 1), "tgroup-batch": reshape("tgroup", B + 1, TS),
             "first+last": both(reshape("tdesc", B, TS, 4), reshape("tgroup", B, TS + 1))})

W["orbAnglesBatch"] = dict(
    base=lambda: dict(pyramids=z(U8, B, 6, 16), kp=z(I32, B, S), counts=z(I32, B)),
    good={"defaults": put(), "angles-given": put(angles=lambda: z(U8, B, S))},
    refused={"kp-batch": reshape("kp", B + 1, S)})

W["selectMatchesBatch"] = dict(
    base=lambda: dict(idx=z(I32, B, S), dist=z(I32, B, S), dist2=z(I32, B, S), qcounts=z(I32, B), tcounts=z(I32, B)),
    good={
        "defaults": put(),
        "angles-back-status-hist": put(qangle=lambda: z(U8, B, S), tangle=lambda: z(U8, B, TS), back_idx=lambda: z(I32, B, TS),
                                       want_status=True, want_hist=True),
        "parameters": put(qangle=lambda: z(U8, B, S), tangle=lambda: z(U8, B, TS), max_dist=33, ratio=(7, 9), unique=False,
                          rot_keep=2, rot_min_pct=12, t_stride=TS),
        "no-ratio-no-angles": put(ratio=None, dist2=None, rot_keep=2, t_stride=11),
        "outputs-given": put(sel_q=lambda: z(I32, B, S), sel_t=lambda: z(I32, B, S), nsel=lambda: z(I32, B),
                             status=lambda: z(U8, B, S), rot_hist=lambda: z(I32, B, 30)),
    },
    refused={
        "qangle-alone": put(qangle=lambda: z(U8, B, S)),
        "tangle-alone": put(tangle=lambda: z(U8, B, TS)),
        "t_stride-against-tangle": put(qangle=lambda: z(U8, B, S), tangle=lambda: z(U8, B, TS), t_stride=TS + 1),
        "back_idx-against-tangle": put(qangle=lambda: z(U8, B, S), tangle=lambda: z(U8, B, TS), back_idx=lambda: z(I32, B, TS + 1)),
        "first+last": put(qangle=lambda: z(U8, B, S), back_idx=lambda: z(I32, B, TS), t_stride=TS + 1),
    })

_two_view = lambda: dict(p1_q8=z(I32, B, S, 2), p2_q8=z(I32, B, S, 2), counts=z(I32, B))
_long_matches = both(reshape("p1_q8", B, 16385, 2), reshape("p2_q8", B, 16385, 2))

W["twoViewRansacBatch"] = dict(
    base=lambda: dict(_two_view(), model="F"),
    good={
        "defaults": put(),
        "parameters": put(model="H", hypotheses=7, seed=0x123456789, sigma_q8=300),
        "model-1": put(model=1),
        "counts-not-checked": put(counts=lambda: z(I64, B + 1, 3)),
        "outputs-given": put(best=lambda: z(I32, B), score=lambda: z(I32, B), ninliers=lambda: z(I32, B),
                             inlier=lambda: z(U8, B, S), model_n=lambda: z(F32, B, 9), stats=lambda: z(I64, B, 8)),
    },
    refused={
        "model": put(model="X"),
        "p1_q8-dtype": retype("p1_q8", I64), "p1_q8-rank": reshape("p1_q8", B, S), "p1_q8-extent": reshape("p1_q8", B, S, 3),
        "p2_q8-dtype": retype("p2_q8", I64), "p2_q8-shape": reshape("p2_q8", B, S + 1, 2),
        "stride-limit": _long_matches,
        "first+last": both(put(model="X"), _long_matches),
    })

W["twoViewReconstructBatch"] = dict(
    base=lambda: dict(_two_view(), cam=z(F32, B, 4), cand=z(F32, B, 3, 12)),
    good={
        "defaults": put(),
        "mask": put(mask=lambda: z(U8, B, S)),
        "counts-uint32": put(counts=lambda: z(U32, B)),
        "parameters": put(sigma_q8=300, min_parallax_deg=2.5, cos_point=0.9999, min_good=40, min_good_pct=80, similar_pct=60,
                          parallax_rank=41),
        "one-candidate": reshape("cand", B, 1, 12), "eight-candidates": reshape("cand", B, 8, 12),
        "outputs-given": put(best=lambda: z(I32, B), status=lambda: z(I32, B), ngood=lambda: z(I32, B, 8),
                             npar=lambda: z(I32, B, 8), pose_out=lambda: z(F32, B, 12), xw=lambda: z(F32, B, S, 3),
                             point=lambda: z(U8, B, S)),
    },
    refused={
        "p1_q8-dtype": retype("p1_q8", I64), "p1_q8-rank": reshape("p1_q8", B, S), "p1_q8-extent": reshape("p1_q8", B, S, 3),
        "p2_q8-dtype": retype("p2_q8", I64), "p2_q8-shape": reshape("p2_q8", B, S + 1, 2),
        "stride-limit": _long_matches,
        "cand-rank": reshape("cand", B, 36), "cand-batch": reshape("cand", B + 1, 3, 12), "cand-extent": reshape("cand", B, 3, 13),
        "no-candidate": reshape("cand", B, 0, 12), "nine-candidates": reshape("cand", B, 9, 12),
        **refusals(("p1_q8", "p2_q8", "counts", "cam", "cand"),
                   dict(counts=(I64, (B + 1,)), cam=(F64, (B, 5)), cand=(F64, None))),
        **with_first(put(mask=lambda: z(U8, B, S)), refusals(("mask",), dict(mask=(I32, (B, S + 1))))),
        "sigma_q8-0": put(sigma_q8=0), "sigma_q8-4097": put(sigma_q8=4097),
        "min_parallax_deg-100": put(min_parallax_deg=100.0),
        "cos_point-0": put(cos_point=0.0), "cos_point-above-1": put(cos_point=1.5),
        "min_good-0": put(min_good=0), "min_good-16385": put(min_good=16385),
        "min_good_pct-below": put(min_good_pct=-1), "min_good_pct-101": put(min_good_pct=101),
        "similar_pct-0": put(similar_pct=0), "similar_pct-101": put(similar_pct=101),
        "parallax_rank-0": put(parallax_rank=0), "parallax_rank-16385": put(parallax_rank=16385),
        "first+last": both(retype("p1_q8", I64), put(parallax_rank=0)),
    })

# the level arguments of the pose and Sim(3) calls
_table = [1.0, 0.5, 0.25]
_level = put(level=lambda: z(U8, B, S), inv_sigma2=_table)
_levels = put(level1=lambda: z(U8, B, S), level2=lambda: z(U8, B, S), inv_sigma2=_table)


def _table_cases(levels):
    return {
        "table-one-entry": both(levels, put(inv_sigma2=np.float64(0.5))),
        "table-16-entries": both(levels, put(inv_sigma2=lambda: np.arange(1, 17, dtype=np.float64).reshape(4, 4))),
        "table-strided": both(levels, put(inv_sigma2=lambda: np.arange(1, 7, dtype=np.float32)[::2])),
        "table-transposed": both(levels, put(inv_sigma2=lambda: np.arange(1, 7, dtype=np.float64).reshape(2, 3).T)),
    }


def _table_refusals(levels):
    return {"table-empty": both(levels, put(inv_sigma2=[])), "table-17-entries": both(levels, put(inv_sigma2=[1.0] * 17))}


_long_points = both(reshape("xw", B, 16385, 3), reshape("obs_q8", B, 16385, 3))

W["poseRefineBatch"] = dict(
    base=lambda: dict(pose=z(F32, B, 12), cam=z(F32, B, 5), xw=z(F32, B, S, 3), obs_q8=z(I32, B, S, 3), counts=z(I32, B)),
    good={
        "defaults": put(),
        "level": _level, **_table_cases(_level),
        "counts-uint32": put(counts=lambda: z(U32, B)),
        "parameters": put(rounds=3, iters=7, huber_rounds=2, min_obs=6, eps=1e-4),
        "outputs-given": put(pose_out=lambda: z(F32, B, 12), inlier=lambda: z(U8, B, S), ninliers=lambda: z(I32, B),
                             cost=lambda: z(F64, B), status=lambda: z(I32, B)),
        "in-place": lambda b: dict(pose_out=b["pose"]),
    },
    refused={
        "pose-numpy": lambda b: dict(pose=b["pose"].numpy()),
        "pose-rank": reshape("pose", B * 12), "xw-rank": reshape("xw", B, S * 3), "xw-batch": reshape("xw", B + 1, S, 3),
        **refusals(("pose", "cam", "xw", "obs_q8", "counts"),
                   dict(pose=(F64, (B, 13)), cam=(F64, (B, 4)), xw=(F64, (B, S, 4)), obs_q8=(I64, (B, S + 1, 3)),
                        counts=(I64, (B + 1,)))),
        "cam-batch": reshape("cam", B + 1, 5),
        "stride-limit": _long_points,
        "level-alone": put(level=lambda: z(U8, B, S)), "inv_sigma2-alone": put(inv_sigma2=_table),
        **with_first(_level, refusals(("level",), dict(level=(I32, (B, S + 1))))),
        **_table_refusals(_level),
        "first+last": both(_level, retype("pose", F64), stride_of("level")),
    })

W["pnpRansacBatch"] = dict(
    base=lambda: dict(cam=z(F32, B, 5), xw=z(F32, B, S, 3), obs_q8=z(I32, B, S, 3), counts=z(I32, B)),
    good={
        "defaults": put(),
        "level": _level, **_table_cases(_level),
        "counts-uint32": put(counts=lambda: z(U32, B)),
        "parameters": put(hypotheses=7, seed=0x123456789, min_inliers=4),
        "outputs-given": put(best=lambda: z(I32, B), score=lambda: z(I32, B), ninliers=lambda: z(I32, B),
                             inlier=lambda: z(U8, B, S), pose_out=lambda: z(F32, B, 12), status=lambda: z(I32, B)),
    },
    refused={
        "cam-rank": reshape("cam", B * 5), "xw-rank": reshape("xw", B, S * 3), "xw-batch": reshape("xw", B + 1, S, 3),
        **refusals(("cam", "xw", "obs_q8", "counts"),
                   dict(cam=(F64, (B, 4)), xw=(F64, (B, S, 4)), obs_q8=(I64, (B, S + 1, 3)), counts=(I64, (B + 1,)))),
        "stride-limit": _long_points,
        "level-alone": put(level=lambda: z(U8, B, S)), "inv_sigma2-alone": put(inv_sigma2=_table),
        **with_first(_level, refusals(("level",), dict(level=(I32, (B, S + 1))))),
        **_table_refusals(_level),
        "first+last": both(_level, retype("cam", F64), stride_of("level")),
    })

_sim3 = lambda: dict(cam1=z(F32, B, 5), cam2=z(F32, B, 5), x1=z(F32, B, S, 3), x2=z(F32, B, S, 3), obs1_q8=z(I32, B, S, 3),
                     obs2_q8=z(I32, B, S, 3), counts=z(I32, B))
_long_pairs = both(reshape("x1", B, 16385, 3), reshape("x2", B, 16385, 3), reshape("obs1_q8", B, 16385, 3),
                   reshape("obs2_q8", B, 16385, 3))
_sim3_names = ("cam1", "cam2", "x1", "x2", "obs1_q8", "obs2_q8", "counts")
_sim3_wrong = dict(cam1=(F64, (B, 4)), cam2=(F64, (B + 1, 5)), x1=(F64, (B, S, 4)), x2=(F64, (B, S + 1, 3)),
                   obs1_q8=(I64, (B, S + 1, 3)), obs2_q8=(I64, (B, S, 2)), counts=(I64, (B + 1,)))
_sim3_levels = {
    "level1-alone": put(level1=lambda: z(U8, B, S)), "level2-alone": put(level2=lambda: z(U8, B, S)),
    "inv_sigma2-alone": put(inv_sigma2=_table), "levels-without-table": put(level1=lambda: z(U8, B, S), level2=lambda: z(U8, B, S)),
    "level1-and-table": put(level1=lambda: z(U8, B, S), inv_sigma2=_table),
    **with_first(_levels, refusals(("level1", "level2"), dict(level1=(I32, (B, S + 1)), level2=(I32, (B + 1, S))))),
    **_table_refusals(_levels),
}

W["sim3RansacBatch"] = dict(
    base=_sim3,
    good={
        "defaults": put(),
        "levels": _levels, **_table_cases(_levels),
        "counts-uint32": put(counts=lambda: z(U32, B)),
        "parameters": put(hypotheses=7, seed=0x123456789, min_inliers=4, fixed_scale=True),
        "outputs-given": put(best=lambda: z(I32, B), score=lambda: z(I32, B), ninliers=lambda: z(I32, B),
                             inlier=lambda: z(U8, B, S), sim_out=lambda: z(F32, B, 13), status=lambda: z(I32, B)),
    },
    refused={
        "cam1-rank": reshape("cam1", B * 5), "x1-rank": reshape("x1", B, S * 3), "x1-batch": reshape("x1", B + 1, S, 3),
        **refusals(_sim3_names, _sim3_wrong),
        "stride-limit": _long_pairs,
        **_sim3_levels,
        "first+last": both(_levels, retype("cam1", F64), stride_of("level2")),
    })

W["sim3RefineBatch"] = dict(
    base=lambda: dict(sim_in=z(F32, B, 13), **_sim3()),
    good={
        "defaults": put(),
        "levels": _levels, **_table_cases(_levels),
        "mask": put(mask=lambda: z(U8, B, S)),
        "counts-uint32": put(counts=lambda: z(U32, B)),
        "parameters": put(rounds=3, iters=7, huber_rounds=1, min_obs=3, th2=8.5, fixed_scale=True, eps=1e-4),
        "outputs-given": put(sim_out=lambda: z(F32, B, 13), inlier=lambda: z(U8, B, S), ninliers=lambda: z(I32, B),
                             cost=lambda: z(F64, B), status=lambda: z(I32, B)),
        "in-place": lambda b: dict(sim_out=b["sim_in"]),
    },
    refused={
        "sim_in-rank": reshape("sim_in", B * 13), "x1-rank": reshape("x1", B, S * 3), "x1-batch": reshape("x1", B + 1, S, 3),
        **refusals(("sim_in",) + _sim3_names, dict(sim_in=(F64, (B, 12)), **_sim3_wrong)),
        "stride-limit": _long_pairs,
        **_sim3_levels,
        **with_first(put(mask=lambda: z(U8, B, S)), refusals(("mask",), dict(mask=(I32, (B, S + 1))))),
        "first+last": both(put(mask=lambda: z(U8, B, S)), retype("sim_in", F64), stride_of("mask")),
    })

_tables2 = put(level_scale=[1.0, 1.5, 2.25], level_sigma2=[1.0, 2.25, 5.0625])
_epi_names = ("qgroup", "tgroup", "qobs_q8", "tobs_q8", "qlevel", "tlevel", "f12", "epipole")
_masks = put(qmask=lambda: z(U8, B, S), tmask=lambda: z(U8, B, TS))

W["matchEpipolarBatch"] = dict(
    base=lambda: dict(qdesc=z(I32, B, S, 8), qgroup=z(I32, B, S), qobs_q8=z(I32, B, S, 3), qlevel=z(U8, B, S), qcounts=z(I32, B),
                      tdesc=z(I32, B, TS, 8), tgroup=z(I32, B, TS), tobs_q8=z(I32, B, TS, 3), tlevel=z(U8, B, TS),
                      tcounts=z(I32, B), ngroups=10, f12=z(F32, B, 9), epipole=z(F32, B, 2)),
    good={
        "defaults": put(),
        "masks": _masks,
        "tables": _tables2,
        "tables-strided": put(level_scale=lambda: np.arange(1, 7, dtype=np.float32)[::2],
                              level_sigma2=lambda: np.arange(1, 7, dtype=np.float64).reshape(2, 3).T[:, 0]),
        "pyramid": put(nlevels=4, scale=1.5),
        "groups-of-another-type": both(retype("qgroup", I16), retype("tgroup", I64)),
        "parameters": put(ngroups=33, chi2=5.5, epipole_r2=64.0),
        "outputs-given": put(idx=lambda: z(I32, B, S), dist=lambda: z(I32, B, S), dist2=lambda: z(I32, B, S)),
    },
    refused={
        "tdesc-batch": reshape("tdesc", B + 1, TS, 8), "tdesc-words": reshape("tdesc", B, TS, 4),
        **refusals(_epi_names, dict(qgroup=(None, (B, S + 1)), tgroup=(None, (B, S)), qobs_q8=(I64, (B, S, 2)),
                                    tobs_q8=(I64, (B, S, 3)), qlevel=(I32, (B, TS)), tlevel=(I32, (B, S)),
                                    f12=(F64, (B, 8)), epipole=(F64, (B + 1, 2)))),
        **with_first(_masks, refusals(("qmask", "tmask"), dict(qmask=(I32, (B, TS)), tmask=(I32, (B, S))))),
        "level_sigma2-alone": put(level_sigma2=[1.0, 2.25]), "level_scale-alone": put(level_scale=[1.0, 1.5]),
        "tables-empty": put(level_sigma2=[], level_scale=[]),
        "tables-17-entries": put(level_sigma2=[1.0] * 17, level_scale=[1.0] * 17),
        "tables-of-unequal-length": put(level_sigma2=[1.0, 2.25], level_scale=[1.0, 1.5, 2.25]),
        "nlevels-17": put(nlevels=17),
        "first+last": both(reshape("tdesc", B, TS, 4), put(level_sigma2=[1.0, 2.25], level_scale=[1.0, 1.5, 2.25])),
    })

_tri_names = ("pose1", "pose2", "cam1", "cam2", "obs1_q8", "obs2_q8", "level1", "level2", "counts")

W["triangulateBatch"] = dict(
    base=lambda: dict(pose1=z(F32, B, 12), pose2=z(F32, B, 12), cam1=z(F32, B, 5), cam2=z(F32, B, 5), obs1_q8=z(I32, B, S, 3),
                      obs2_q8=z(I32, B, S, 3), level1=z(U8, B, S), level2=z(U8, B, S), counts=z(I32, B)),
    good={
        "defaults": put(),
        "tables": _tables2,
        "tables-strided": put(level_scale=lambda: np.arange(1, 7, dtype=np.float32)[::2],
                              level_sigma2=lambda: np.arange(1, 7, dtype=np.float64).reshape(2, 3).T[:, 0]),
        "pyramid": put(nlevels=4, scale=1.5),
        "counts-uint32": put(counts=lambda: z(U32, B)),
        "parameters": put(cos_min_parallax=0.999, chi2_mono=5.5, chi2_stereo=7.5, ratio_factor=1.75),
        "no-normal": put(want_normal=False), "no-drange": put(want_drange=False),
        "normal-given-though-not-wanted": put(want_normal=False, normal=lambda: z(F32, B, S, 3)),
        "outputs-given": put(xw=lambda: z(F32, B, S, 3), status=lambda: z(U8, B, S), normal=lambda: z(F32, B, S, 3),
                             drange=lambda: z(F32, B, S, 2), npoints=lambda: z(I32, B)),
    },
    refused={
        "pose1-rank": reshape("pose1", B * 12), "obs1_q8-rank": reshape("obs1_q8", B, S * 3),
        "obs1_q8-batch": reshape("obs1_q8", B + 1, S, 3),
        **refusals(_tri_names, dict(pose1=(F64, (B, 13)), pose2=(F64, (B + 1, 12)), cam1=(F64, (B, 4)), cam2=(F64, (B + 1, 5)),
                                    obs1_q8=(I64, (B, S, 2)), obs2_q8=(I64, (B, S + 1, 3)), level1=(I32, (B, S + 1)),
                                    level2=(I32, (B + 1, S)), counts=(I64, (B + 1,)))),
        "stride-limit": both(reshape("obs1_q8", B, 16385, 3), reshape("obs2_q8", B, 16385, 3)),
        "level_scale-alone": put(level_scale=[1.0, 1.5]), "level_sigma2-alone": put(level_sigma2=[1.0, 2.25]),
        "tables-empty": put(level_sigma2=[], level_scale=[]),
        "tables-17-entries": put(level_sigma2=[1.0] * 17, level_scale=[1.0] * 17),
        "tables-of-unequal-length": put(level_sigma2=[1.0, 2.25], level_scale=[1.0, 1.5, 2.25]),
        "nlevels-17": put(nlevels=17),
        "first+last": both(retype("pose1", F64), put(level_sigma2=[1.0, 2.25], level_scale=[1.0, 1.5, 2.25])),
    })

_ba_names = ("poses", "cams", "kf_counts", "kf_free", "xw", "pt_counts", "obs_q8", "obs_kf", "obs_pt", "counts")
_ba_long = both(reshape("obs_q8", B, 16385, 3), reshape("obs_kf", B, 16385), reshape("obs_pt", B, 16385))

W["localBundleAdjustBatch"] = dict(
    base=lambda: dict(poses=z(F32, B, KF, 12), cams=z(F32, B, KF, 5), kf_counts=z(I32, B), kf_free=z(I32, B), xw=z(F32, B, PT, 3),
                      pt_counts=z(I32, B), obs_q8=z(I32, B, S, 3), obs_kf=z(U8, B, S), obs_pt=z(I16, B, S), counts=z(I32, B)),
    good={
        "defaults": put(),
        "level": _level, **_table_cases(_level),
        "words-unsigned": put(obs_pt=lambda: z(U16, B, S), kf_counts=lambda: z(U32, B), kf_free=lambda: z(U32, B),
                              pt_counts=lambda: z(U32, B), counts=lambda: z(U32, B)),
        "parameters": put(rounds=3, iters=(4, 6, 8), huber_rounds=2, min_obs=6, eps=1e-4),
        "iters-one-number": put(iters=7), "iters-four": put(rounds=4, iters=[1, 2, 3, 4]),
        "outputs-given": put(poses_out=lambda: z(F32, B, KF, 12), xw_out=lambda: z(F32, B, PT, 3), inlier=lambda: z(U8, B, S),
                             ninliers=lambda: z(I32, B), cost=lambda: z(F64, B), status=lambda: z(I32, B)),
        "in-place": lambda b: dict(poses_out=b["poses"], xw_out=b["xw"]),
    },
    refused={
        "poses-rank": reshape("poses", B, KF * 12), "xw-rank": reshape("xw", B, PT * 3), "xw-batch": reshape("xw", B + 1, PT, 3),
        "obs_q8-rank": reshape("obs_q8", B, S * 3), "obs_q8-batch": reshape("obs_q8", B + 1, S, 3),
        **refusals(_ba_names, dict(poses=(F64, (B, KF, 13)), cams=(F64, (B, KF + 1, 5)), xw=(F64, (B, PT, 4)),
                                   obs_q8=(I64, (B, S, 2)), obs_kf=(I32, (B, S + 1)), obs_pt=(I32, (B, S + 1)),
                                   kf_counts=(I64, (B + 1,)), kf_free=(I64, (B + 1,)), pt_counts=(I64, (B + 1,)),
                                   counts=(I64, (B + 1,)))),
        "key-frame-limit": both(reshape("poses", B, 33, 12), reshape("cams", B, 33, 5)),
        "point-limit": reshape("xw", B, 4097, 3),
        "stride-limit": _ba_long,
        "level-alone": put(level=lambda: z(U8, B, S)), "inv_sigma2-alone": put(inv_sigma2=_table),
        **with_first(_level, refusals(("level",), dict(level=(I32, (B, S + 1))))),
        **_table_refusals(_level),
        "iters-too-few": put(rounds=3, iters=(5, 10)), "iters-five": put(iters=(1, 2, 3, 4, 5)),
        "first+last": both(retype("poses", F64), put(iters=(1, 2, 3, 4, 5))),
    })

_pg_names = ("sims", "v_counts", "fixed", "edges", "meas", "e_counts", "inc_ptr", "inc")
_weight = put(weight=lambda: z(F32, B, E))

W["poseGraphBatch"] = dict(
    base=lambda: dict(sims=z(F32, B, V, 13), v_counts=z(I32, B), fixed=z(U8, B, V), edges=z(I32, B, E, 2), meas=z(F32, B, E, 13),
                      weight=None, e_counts=z(I32, B), inc_ptr=z(I32, B, V + 1), inc=z(I32, B, 2 * E)),
    good={
        "defaults": put(),
        "weight": _weight,
        "words-unsigned": put(edges=lambda: z(U32, B, E, 2), v_counts=lambda: z(U32, B), e_counts=lambda: z(U32, B),
                              inc_ptr=lambda: z(U32, B, V + 1), inc=lambda: z(U32, B, 2 * E)),
        "parameters": put(iters=7, cg_iters=100, cg_tol=1e-4, eps=1e-6),
        "outputs-given": put(sims_out=lambda: z(F32, B, V, 13), cost=lambda: z(F64, B), status=lambda: z(I32, B)),
        "in-place": lambda b: dict(sims_out=b["sims"]),
    },
    refused={
        "sims-rank": reshape("sims", B, V * 13), "edges-rank": reshape("edges", B, E * 2), "edges-batch": reshape("edges", B + 1, E, 2),
        **refusals(_pg_names, dict(sims=(F64, (B, V, 12)), edges=(I64, (B, E, 3)), fixed=(I32, (B, V + 1)), meas=(F64, (B, E + 1, 13)),
                                   v_counts=(I64, (B + 1,)), e_counts=(I64, (B + 1,)), inc_ptr=(I64, (B, V)),
                                   inc=(I64, (B, 2 * E + 1)))),
        "vertex-limit": reshape("sims", B, 4097, 13), "edge-limit": reshape("edges", B, 16385, 2),
        **with_first(_weight, refusals(("weight",), dict(weight=(F64, (B, E + 1))))),
        "first+last": both(_weight, retype("sims", F64), stride_of("weight")),
    })

_cmp_names = ("xw", "ref", "pt_counts", "sims_old", "sims_new", "v_counts")

W["correctMapPointsBatch"] = dict(
    base=lambda: dict(xw=z(F32, B, PT, 3), ref=z(I16, B, PT), pt_counts=z(I32, B), sims_old=z(F32, B, V, 13),
                      sims_new=z(F32, B, V, 13), v_counts=z(I32, B)),
    good={
        "defaults": put(),
        "words-unsigned": put(ref=lambda: z(U16, B, PT), pt_counts=lambda: z(U32, B), v_counts=lambda: z(U32, B)),
        "outputs-given": put(xw_out=lambda: z(F32, B, PT, 3), status=lambda: z(U8, B, PT)),
        "in-place": lambda b: dict(xw_out=b["xw"]),
    },
    refused={
        "xw-rank": reshape("xw", B, PT * 3), "sims_old-rank": reshape("sims_old", B, V * 13),
        "sims_old-batch": both(reshape("sims_old", B + 1, V, 13), reshape("sims_new", B + 1, V, 13)),
        **refusals(_cmp_names, dict(xw=(F64, (B, PT, 4)), ref=(I32, (B, PT + 1)), sims_old=(F64, (B, V, 12)),
                                    sims_new=(F64, (B, V + 1, 13)), pt_counts=(I64, (B + 1,)), v_counts=(I64, (B + 1,)))),
        "first+last": both(retype("xw", F64), stride_of("v_counts")),
    })

W["bowWeightBatch"] = dict(
    base=lambda: dict(bow_word=z(I32, B, S), bow_tf=z(I32, B, S), bow_n=z(I32, B), nwords=100),
    good={
        "defaults": put(),
        "idf": put(idf=lambda: z(I32, 50), nwords=None),
        "idf-and-fewer-words": put(idf=lambda: z(I32, 50), nwords=40),
        "most-words": put(nwords=1 << 24),
        "output-given": put(bow_weight=lambda: z(I32, B, S)),
    },
    refused={
        "bow_word-rank": reshape("bow_word", B * S),
        "stride-limit": both(reshape("bow_word", B, 16385), reshape("bow_tf", B, 16385)),
        "bow_tf-shape": reshape("bow_tf", B, S + 1), "bow_n-shape": reshape("bow_n", B + 1),
        "idf-rank": put(idf=lambda: z(I32, 5, 10), nwords=None),
        "nwords-above-idf": put(idf=lambda: z(I32, 50), nwords=51),
        "nwords-missing": put(nwords=None),
        "nwords-0": put(nwords=0), "nwords-above-2^24": put(nwords=(1 << 24) + 1),
        "bow_weight-shape": put(bow_weight=lambda: z(I32, B, S + 1)),
        "first+last": both(reshape("bow_word", B * S), put(bow_weight=lambda: z(I32, B, S + 1))),
    })

WRAPPERS = tuple(W)
# helpers whose refusals are the wrapper's own (the completeness check of the recorder reads them with the wrapper)
CHECKED_WITH = {"bowWeightBatch": ("_check_bow_rows",), "matchHammingWindowBatch": ("_window_tables",),
                "matchHammingScaledWindowBatch": ("_scaled_tables", "_window_tables")}


# ---- running a case and writing down what happened ------------------------------------------------------------------------
def _argument(a, ctx, named, returned):
    if a is ctx.h:
        return "ctx"
    if a is None or (isinstance(a, int) and a == 0):
        return "null"
    if isinstance(a, ctypes.Array):
        raw = bytes(a)
        return ["%08x" % w for w in struct.unpack(f"<{len(raw) // 4}I", raw)]
    if hasattr(a, "_obj"):                                      # ctypes.byref(struct)
        return bytes(a._obj).hex()
    assert isinstance(a, int), a
    for name, t in named.items():
        if t.data_ptr() == a:
            return name
    for i, t in enumerate(returned):
        if t is not None and t.data_ptr() == a:
            return f"new:{i}"
    assert a < 1 << 32, "a pointer to a tensor that was neither passed in nor returned"
    return a


def run(wrapper, kind, case):
    """The record of one case: {"calls": ..., "returns": ...} for a good call, the message for a refused one."""
    spec = W[wrapper]
    call = spec["base"]()
    call.update(spec[kind][case](call))
    ctx = Recorder()
    fn = getattr(fe, wrapper)
    if kind == "refused":
        with pytest.raises(ValueError) as e:
            fn(**call, ctx=ctx)
        assert ctx.calls == [] and ctx.checked == []
        return str(e.value)
    got = fn(**call, ctx=ctx)
    returned = got if isinstance(got, tuple) else (got,)
    named = {k: v for k, v in call.items() if isinstance(v, torch.Tensor)}
    assert all(t.numel() for t in named.values())               # (an empty tensor has the address 0)
    who = lambda t: next((k for k, v in named.items() if v is t), None)
    return {
        "calls": [{"fn": name, "args": [_argument(a, ctx, named, returned) for a in args]} for name, args in ctx.calls],
        "check": ctx.checked,
        "returns": [None if t is None else {"dtype": str(t.dtype).replace("torch.", ""), "shape": list(t.shape), "is": who(t)}
                    for t in returned],
    }


CASES = [(w, kind, case) for w in WRAPPERS for kind in ("good", "refused") for case in W[w][kind]]


@pytest.fixture(scope="module")
def record():
    with open(RECORD) as f:
        return json.load(f)


@pytest.mark.parametrize("wrapper,kind,case", CASES, ids=["-".join(c) for c in CASES])
def test_wrapper_passes_and_refuses_as_recorded(record, wrapper, kind, case):
    assert run(wrapper, kind, case) == record["wrappers"][wrapper][kind][case]


def test_record_holds_these_cases_and_reaches_every_refusal(record):
    """The record has exactly the cases above, and per wrapper as many of its `raise ValueError` sites are reached by a recorded
    message as the recorder counted in the source it was made from, less those it lists as unreachable."""
    assert list(record["wrappers"]) == list(WRAPPERS)
    for w in WRAPPERS:
        for kind in ("good", "refused"):
            assert list(record["wrappers"][w][kind]) == list(W[w][kind]), (w, kind)
        sites = record["sites"][w]
        assert sites["reached"] == sites["raise ValueError"] - len(sites["unreachable"]), w
        assert all(len(c["calls"]) == 1 for c in record["wrappers"][w]["good"].values())


# ---- the numpy path of the three wrappers that have one: it ends on the device ---------------------------------------------
@pytest.mark.gpu
def test_numpy_inputs_equal_tensor_inputs(gpu_ctx):
    """pnpRansacBatch, sim3RansacBatch and sim3RefineBatch take numpy arrays and move them to the current device: the same
    arrays as numpy and as device tensors give outputs on the device that are equal byte for byte, wherever the calls write
    (the kernels are deterministic; the values are random finite numbers, not a scene)."""
    rng = np.random.default_rng(5)
    batch, stride = 2, 16
    pts = lambda: rng.uniform(-2.0, 2.0, (batch, stride, 3)).astype(np.float32) + np.float32([0, 0, 6])
    obs = lambda: np.concatenate([rng.integers(0, 640 * 256, (batch, stride, 2)),
                                  np.full((batch, stride, 1), fe.POSE_MONO)], axis=2).astype(np.int32)
    cam = lambda: np.tile(np.float32([500, 500, 320, 240, 40]), (batch, 1))
    lvl = lambda: rng.integers(0, 3, (batch, stride)).astype(np.uint8)
    counts, table = np.array([16, 5], np.int32), fe.poseLevelWeights(3)
    sim = np.tile(np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, -0.1, 0.2, 1.1]), (batch, 1))
    pair = dict(cam1=cam(), cam2=cam(), x1=pts(), x2=pts(), obs1_q8=obs(), obs2_q8=obs(), counts=counts, level1=lvl(), level2=lvl())
    calls = (
        (fe.pnpRansacBatch, dict(cam=cam(), xw=pts(), obs_q8=obs(), counts=counts, level=lvl()),
         dict(inv_sigma2=table, hypotheses=8, min_inliers=4)),
        (fe.sim3RansacBatch, pair, dict(inv_sigma2=table, hypotheses=8, min_inliers=4)),
        (fe.sim3RefineBatch, dict(sim_in=sim, mask=(rng.random((batch, stride)) < 0.8).astype(np.uint8), **pair),
         dict(inv_sigma2=table, min_obs=3)),
    )
    for fn, arrays, kw in calls:
        from_numpy = fn(**arrays, **kw, ctx=gpu_ctx)
        from_tensors = fn(**{k: torch.from_numpy(a).to("cuda") for k, a in arrays.items()}, **kw, ctx=gpu_ctx)
        gpu_ctx.synchronize()
        assert len(from_numpy) == len(from_tensors) >= 5
        for a, b in zip(from_numpy, from_tensors):
            assert a.is_cuda and b.is_cuda and a.dtype == b.dtype and a.shape == b.shape, fn.__name__
            a, b = a.cpu().numpy(), b.cpu().numpy()
            if a.shape == (batch, stride):                   # inlier: the calls do not write at and beyond counts[b]
                a, b = (np.where(np.arange(stride) < counts[:, None], x, 0) for x in (a, b))
            assert a.tobytes() == b.tobytes(), fn.__name__


# ---- the recorder ------------------------------------------------------------------------------------------------------
def _raise_sites(wrapper):
    """[(line, regex of the message)] of every `raise ValueError(...)` in the wrapper's source (and its CHECKED_WITH helpers): an
    f-string's fields match anything."""
    import ast
    import inspect
    import re
    sites = []
    for name in (wrapper,) + CHECKED_WITH.get(wrapper, ()):
        fn = getattr(fe, name)
        first = inspect.getsourcelines(fn)[1]
        for node in ast.walk(ast.parse(inspect.getsource(fn))):
            if not (isinstance(node, ast.Raise) and isinstance(node.exc, ast.Call) and getattr(node.exc.func, "id", "") == "ValueError"):
                continue
            message = node.exc.args[0]
            while isinstance(message, ast.BinOp):                # (text + an optional tail: the text)
                message = message.left
            parts = [re.escape(leaf.value) for leaf in ast.walk(message) if isinstance(leaf, ast.Constant) and leaf.value]
            sites.append((first + node.lineno - 1, ".*".join(parts)))
    return sites


def main(unreachable=()):
    import re
    import subprocess
    from conftest import ROOT
    commit = subprocess.run(["git", "-C", ROOT, "log", "-1", "--format=%h %s", "--", "pislam_amd/frontend.py"],
                            capture_output=True, text=True).stdout.strip()
    out = {"recorded from": f"pislam_amd/frontend.py as of {commit}", "sites": {}, "wrappers": {}}
    for w in WRAPPERS:
        out["wrappers"][w] = {kind: {case: run(w, kind, case) for case in W[w][kind]} for kind in ("good", "refused")}
        messages = set(out["wrappers"][w]["refused"].values())
        sites = _raise_sites(w)
        missed = [f"line {line}: {rx}" for line, rx in sites if not any(re.fullmatch(".*" + rx + ".*", m, re.S) for m in messages)]
        listed = [s for s in missed if any(u in s for u in unreachable)]
        assert missed == listed, (w, missed)
        out["sites"][w] = {"raise ValueError": len(sites), "reached": len(sites) - len(missed), "unreachable": listed,
                           "distinct messages": len(messages)}
    lines = ["{", f' "recorded from": {json.dumps(out["recorded from"])},', ' "sites": {']
    lines += [",\n".join(f"  {json.dumps(w)}: {json.dumps(s)}" for w, s in out["sites"].items()), " },", ' "wrappers": {']
    blocks = []
    for w, kinds in out["wrappers"].items():
        body = []
        for kind, cases in kinds.items():
            rows = ",\n".join(f"    {json.dumps(c)}: {json.dumps(r)}" for c, r in cases.items())
            body.append(f"   {json.dumps(kind)}: {{\n{rows}\n   }}")
        blocks.append(f"  {json.dumps(w)}: {{\n" + ",\n".join(body) + "\n  }")
    lines += [",\n".join(blocks), " }", "}"]
    with open(RECORD, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{RECORD}: {sum(len(W[w]['good']) for w in WRAPPERS)} good calls, {sum(len(W[w]['refused']) for w in WRAPPERS)} refusals")
    for w, s in out["sites"].items():
        print(f"  {w}: {s}")


if __name__ == "__main__":
    main()
