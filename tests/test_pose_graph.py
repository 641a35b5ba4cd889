"""pislam_pose_graph_batch and pislam_map_points_correct_batch: essential-graph optimisation after a loop.

The comments above the two calls in include/pislam_hip.h are the contract.  This file restates them in numpy,
independently of the library (binary64 one operation at a time on arrays; the sums in the stated orders: the edge and
vertex sums by 256 partials and the halving tree, the per-vertex sums entry by entry in ascending order).  The host probe
(tools/probes/graph_host_check.cpp, the library's own arithmetic header under the host compiler) must agree with it on
every output word, the stated Jacobians must agree with central differences, a dense binary64 Levenberg with
differenced Jacobians must reach the same cost and poses, and the library on the GPU must agree with the restatement
(or, for large shapes, with the probe that is pinned to it) on every output word."""
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

F32, F64 = np.float32, np.float64
COUNT_INVALID = 0xFFFFFFFF
PG_FIELDS = ["iters", "cg_iters", "cg_tol", "eps"]
DEFAULT = (20, 256, 1e-6, 1e-9)                # iters, cg_iters, cg_tol, eps
MAX_V, MAX_E = 4096, 16384
LAMBDA_0, LAMBDA_MIN, LAMBDA_MAX = 2.0 ** -10, 2.0 ** -30, 2.0 ** 20
ROT_MIN = 2.0 ** -10
SENT = 0x5A5A5A5A


# ---- the restatement: similarities, residual, Jacobians (arrays [..][13] and [..][7]) -----------------------------------
def mat3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def ref_compose(A, B):
    C = np.empty(np.broadcast(A, B).shape, F64)
    for i in range(3):
        for j in range(3):
            C[..., 3 * i + j] = mat3(A[..., 3 * i], A[..., 3 * i + 1], A[..., 3 * i + 2], B[..., j], B[..., 3 + j], B[..., 6 + j])
        C[..., 9 + i] = A[..., 12] * mat3(A[..., 3 * i], A[..., 3 * i + 1], A[..., 3 * i + 2], B[..., 9], B[..., 10],
                                          B[..., 11]) + A[..., 9 + i]
    C[..., 12] = A[..., 12] * B[..., 12]
    return C


def ref_edge_error(M, Si, Sj):
    G = ref_compose(M, Si)
    E = np.empty_like(G)
    with np.errstate(all="ignore"):
        for a in range(3):
            for b in range(3):
                E[..., 3 * a + b] = mat3(G[..., 3 * a], G[..., 3 * a + 1], G[..., 3 * a + 2], Sj[..., 3 * b], Sj[..., 3 * b + 1],
                                         Sj[..., 3 * b + 2])
        E[..., 12] = G[..., 12] / Sj[..., 12]
        for a in range(3):
            E[..., 9 + a] = G[..., 9 + a] - E[..., 12] * mat3(E[..., 3 * a], E[..., 3 * a + 1], E[..., 3 * a + 2], Sj[..., 9],
                                                              Sj[..., 10], Sj[..., 11])
    return E


def ref_residual(E):
    """(r [..][7], admissible [..])."""
    with np.errstate(all="ignore"):
        c = 1.0 + ((E[..., 0] + E[..., 4]) + E[..., 8])
        r = np.empty(E.shape[:-1] + (7,), F64)
        r[..., 0] = (2.0 * (E[..., 7] - E[..., 5])) / c
        r[..., 1] = (2.0 * (E[..., 2] - E[..., 6])) / c
        r[..., 2] = (2.0 * (E[..., 3] - E[..., 1])) / c
        r[..., 3:6] = E[..., 9:12]
        r[..., 6] = (2.0 * (E[..., 12] - 1.0)) / (E[..., 12] + 1.0)
        return r, c > ROT_MIN


def dot7(a, b):
    with np.errstate(all="ignore"):
        s = a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]
        for k in range(2, 7):
            s = s + a[..., k] * b[..., k]
    return s


def ref_ji(E, M, p):
    o = np.empty(np.broadcast(E[..., :7], p).shape, F64)
    a = [mat3(M[..., 3 * i], M[..., 3 * i + 1], M[..., 3 * i + 2], p[..., 0], p[..., 1], p[..., 2]) for i in range(3)]
    b = [M[..., 12] * mat3(M[..., 3 * i], M[..., 3 * i + 1], M[..., 3 * i + 2], p[..., 3], p[..., 4], p[..., 5]) for i in range(3)]
    c = [M[..., 9 + i] - E[..., 9 + i] for i in range(3)]
    o[..., 0], o[..., 1], o[..., 2] = a
    o[..., 3] = ((c[1] * a[2] - c[2] * a[1]) + b[0]) - p[..., 6] * c[0]
    o[..., 4] = ((c[2] * a[0] - c[0] * a[2]) + b[1]) - p[..., 6] * c[1]
    o[..., 5] = ((c[0] * a[1] - c[1] * a[0]) + b[2]) - p[..., 6] * c[2]
    o[..., 6] = p[..., 6]
    return o


def ref_jj(E, p):
    o = np.empty(np.broadcast(E[..., :7], p).shape, F64)
    for i in range(3):
        o[..., i] = -mat3(E[..., 3 * i], E[..., 3 * i + 1], E[..., 3 * i + 2], p[..., 0], p[..., 1], p[..., 2])
        o[..., 3 + i] = -(E[..., 12] * mat3(E[..., 3 * i], E[..., 3 * i + 1], E[..., 3 * i + 2], p[..., 3], p[..., 4], p[..., 5]))
    o[..., 6] = -p[..., 6]
    return o


def ref_jit(E, M, u):
    o = np.empty(np.broadcast(E[..., :7], u).shape, F64)
    c = [M[..., 9 + i] - E[..., 9 + i] for i in range(3)]
    v = [u[..., 0] - (c[1] * u[..., 5] - c[2] * u[..., 4]), u[..., 1] - (c[2] * u[..., 3] - c[0] * u[..., 5]),
         u[..., 2] - (c[0] * u[..., 4] - c[1] * u[..., 3])]
    for i in range(3):
        o[..., i] = mat3(M[..., i], M[..., 3 + i], M[..., 6 + i], v[0], v[1], v[2])
        o[..., 3 + i] = M[..., 12] * mat3(M[..., i], M[..., 3 + i], M[..., 6 + i], u[..., 3], u[..., 4], u[..., 5])
    o[..., 6] = u[..., 6] - mat3(c[0], c[1], c[2], u[..., 3], u[..., 4], u[..., 5])
    return o


def ref_jjt(E, u):
    o = np.empty(np.broadcast(E[..., :7], u).shape, F64)
    for i in range(3):
        o[..., i] = -mat3(E[..., i], E[..., 3 + i], E[..., 6 + i], u[..., 0], u[..., 1], u[..., 2])
        o[..., 3 + i] = -(E[..., 12] * mat3(E[..., i], E[..., 3 + i], E[..., 6 + i], u[..., 3], u[..., 4], u[..., 5]))
    o[..., 6] = -u[..., 6]
    return o


def ref_jac(side, E, M):
    """The dense Jacobians [n][7][7] of the entries (side [n], E and M [n][13])."""
    n = len(side)
    Ji, Jj = np.zeros((n, 7, 7)), np.zeros((n, 7, 7))
    c = [M[:, 9 + i] - E[:, 9 + i] for i in range(3)]
    for j in range(3):
        Ji[:, 0, j], Ji[:, 1, j], Ji[:, 2, j] = M[:, j], M[:, 3 + j], M[:, 6 + j]
        Ji[:, 3, j] = c[1] * M[:, 6 + j] - c[2] * M[:, 3 + j]
        Ji[:, 4, j] = c[2] * M[:, j] - c[0] * M[:, 6 + j]
        Ji[:, 5, j] = c[0] * M[:, 3 + j] - c[1] * M[:, j]
        for i in range(3):
            Ji[:, 3 + i, 3 + j] = M[:, 12] * M[:, 3 * i + j]
            Jj[:, i, j] = -E[:, 3 * i + j]
            Jj[:, 3 + i, 3 + j] = -(E[:, 12] * E[:, 3 * i + j])
    for i in range(3):
        Ji[:, 3 + i, 6] = -c[i]
    Ji[:, 6, 6], Jj[:, 6, 6] = 1.0, -1.0
    return np.where((side == 0)[:, None, None], Ji, Jj)


def ref_cayley(d):
    a0, a1, a2 = d[..., 0] * 0.5, d[..., 1] * 0.5, d[..., 2] * 0.5
    n = (a0 * a0 + a1 * a1) + a2 * a2
    m, den = 1.0 - n, 1.0 + n
    Q = np.empty(d.shape[:-1] + (9,), F64)
    Q[..., 0] = (m + 2.0 * (a0 * a0)) / den
    Q[..., 1] = (2.0 * (a0 * a1) - 2.0 * a2) / den
    Q[..., 2] = (2.0 * (a0 * a2) + 2.0 * a1) / den
    Q[..., 3] = (2.0 * (a1 * a0) + 2.0 * a2) / den
    Q[..., 4] = (m + 2.0 * (a1 * a1)) / den
    Q[..., 5] = (2.0 * (a1 * a2) - 2.0 * a0) / den
    Q[..., 6] = (2.0 * (a2 * a0) - 2.0 * a1) / den
    Q[..., 7] = (2.0 * (a2 * a1) + 2.0 * a0) / den
    Q[..., 8] = (m + 2.0 * (a2 * a2)) / den
    return Q


def ref_retract(T, d):
    """pislam_sim3_refine_batch's Retract: R' = Q R, t' = k (Q t) + upsilon, s' = k s."""
    with np.errstate(all="ignore"):
        Q = ref_cayley(d)
        k = (2.0 + d[..., 6]) / (2.0 - d[..., 6])
        Tn = np.empty(np.broadcast(T, d[..., :1]).shape, F64)
        for i in range(3):
            for j in range(3):
                Tn[..., 3 * i + j] = mat3(Q[..., 3 * i], Q[..., 3 * i + 1], Q[..., 3 * i + 2], T[..., j], T[..., 3 + j], T[..., 6 + j])
            Tn[..., 9 + i] = k * mat3(Q[..., 3 * i], Q[..., 3 * i + 1], Q[..., 3 * i + 2], T[..., 9], T[..., 10], T[..., 11]) + d[..., 3 + i]
        Tn[..., 12] = k * T[..., 12]
    return Tn


# ---- the restatement: sums, blocks, the solve, the call -------------------------------------------------------------
def ref_tree(v, mask=None):
    """The sum of v[i] (where mask[i]) by 256 partials (i mod 256, ascending i), then the halving tree."""
    p = np.zeros(256)
    with np.errstate(all="ignore"):
        for s in range(0, len(v), 256):
            c = v[s:s + 256]
            m = np.ones(len(c), bool) if mask is None else mask[s:s + 256]
            p[:len(c)] = np.where(m, p[:len(c)] + c, p[:len(c)])
        h = 128
        while h >= 1:
            p[:h] = p[:h] + p[h:2 * h]
            h //= 2
    return p[0]


def ref_factor7(H, s):
    """H [n][7][7] symmetric (full): the factors [n][7][7] and ok [n]."""
    A = H.copy()
    n = len(A)
    ok = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for j in range(7):
            A[:, j, j] = A[:, j, j] * s
        for c in range(7):
            ok &= A[:, c, c] > 0.0
            for r in range(c + 1, 7):
                f = A[:, r, c] / A[:, c, c]
                A[:, r, c + 1:] = A[:, r, c + 1:] - f[:, None] * A[:, c, c + 1:]
                A[:, r, c] = f
    return A, ok


def ref_sol7(fac, b):
    b = b.copy()
    x = np.zeros_like(b)
    with np.errstate(all="ignore"):
        for c in range(7):
            for r in range(c + 1, 7):
                b[:, r] = b[:, r] - fac[:, r, c] * b[:, c]
        for r in range(6, -1, -1):
            t = b[:, r]
            for j in range(r + 1, 7):
                t = t - fac[:, r, j] * x[:, j]
            x[:, r] = t / fac[:, r, r]
    return x


class RefGraph:
    """One graph that passed the structure checks: the entries in index order and by rank within their vertex."""

    def __init__(self, g):
        self.g = g
        self.nv, self.ne = len(g["sims"]), len(g["edges"])
        self.i, self.j = g["edges"][:, 0].astype(np.int64), g["edges"][:, 1].astype(np.int64)
        self.M = g["meas"].astype(F64)
        self.w = np.ones(self.ne) if g.get("weight") is None else g["weight"].astype(F64)
        self.free = g["fixed"] == 0
        ptr, inc = g["inc_ptr"].astype(np.int64), g["inc"].astype(np.int64)
        self.ent_e, self.ent_side = inc >> 1, inc & 1
        self.ent_k = np.repeat(np.arange(self.nv), np.diff(ptr))
        rank = np.arange(len(inc)) - ptr[self.ent_k]
        self.by_rank = [np.flatnonzero(rank == r) for r in range(int(rank.max()) + 1 if len(rank) else 0)]

    def vertex_sums(self, contrib, width):
        """Per vertex, from +0.0, its entries' contributions [2 ne][...] in ascending order."""
        acc = np.zeros((self.nv,) + width)
        with np.errstate(all="ignore"):
            for idx in self.by_rank:
                k = self.ent_k[idx]
                acc[k] = acc[k] + contrib[idx]
        return acc

    def evaluate(self, S):
        E = ref_edge_error(self.M, S[self.i], S[self.j])
        r, adm = ref_residual(E)
        with np.errstate(all="ignore"):
            f = np.where(adm, self.w * dot7(r, r), 0.0)
        return E, ref_tree(f), bool(adm.all())

    def solve(self, S, E, lam, prm, stats):
        """(ok, trial S, dmax)."""
        iters, cg_iters, cg_tol, eps = prm
        free, e, side = self.free, self.ent_e, self.ent_side
        Ee, Me, we = E[e], self.M[e], self.w[e]
        with np.errstate(all="ignore"):
            J = ref_jac(side, Ee, Me)
            h = J[:, 0, :, None] * J[:, 0, None, :]
            for q in range(1, 7):
                h = h + J[:, q, :, None] * J[:, q, None, :]
            H = self.vertex_sums(we[:, None, None] * h, (7, 7))
            r, _ = ref_residual(Ee)
            t = we[:, None] * r
            g = self.vertex_sums(np.where((side == 0)[:, None], ref_jit(Ee, Me, t), ref_jjt(Ee, t)), (7,))
            diag = H[:, np.arange(7), np.arange(7)].copy()
            fac, piv = ref_factor7(H, F64(1.0) + F64(lam))
            if not piv[free].all():
                return False, None, 0.0
            x = np.zeros((self.nv, 7))
            rr = -g
            z = ref_sol7(fac, rr)
            p = np.where(free[:, None], z, 0.0)
            rz = ref_tree(dot7(rr, z), free)
            thr = (F64(cg_tol) * F64(cg_tol)) * rz
            for _ in range(cg_iters):
                if rz <= thr:
                    break
                stats["cg"] += 1
                u = self.w[:, None] * (ref_ji(E, self.M, p[self.i]) + ref_jj(E, p[self.j]))
                ue = u[e]
                Ap = self.vertex_sums(np.where((side == 0)[:, None], ref_jit(Ee, Me, ue), ref_jjt(Ee, ue)), (7,))
                Ap = Ap + (F64(lam) * diag) * p
                pAp = ref_tree(dot7(p, Ap), free)
                if not pAp > 0.0:
                    return False, None, 0.0
                alpha = rz / pAp
                x = x + alpha * p
                rr = rr - alpha * Ap
                z = ref_sol7(fac, rr)
                rz1 = ref_tree(dot7(rr, z), free)
                beta = rz1 / rz
                p = np.where(free[:, None], z + beta * p, 0.0)
                rz = rz1
            d = x[free]
            ok = bool(np.isfinite(d).all()) and bool((np.abs(d[:, 6]) < 2.0).all())
            St = S.copy()
            St[free] = ref_retract(S[free], d)
        return ok, St, float(np.abs(d).max()) if ok else 0.0


def structure_ok(g):
    nv, ne = len(g["sims"]), len(g["edges"])
    ed, ptr, inc = g["edges"].astype(np.int64), g["inc_ptr"].astype(np.int64), g["inc"].astype(np.int64)
    if ne and ((ed >= nv).any() or (ed[:, 0] == ed[:, 1]).any()):
        return False
    if not (g["fixed"] != 0).any():
        return False
    if ptr[0] != 0 or ptr[nv] != 2 * ne or (np.diff(ptr[:nv + 1]) < 0).any():
        return False
    for k in range(nv):
        ent = inc[ptr[k]:ptr[k + 1]]
        if (ent >> 1 >= ne).any() or (ed[ent >> 1, ent & 1] != k).any() or (np.diff(ent) <= 0).any():
            return False
    return True


def ref_graph(g, prm=DEFAULT):
    """The whole call for one graph: dict(status, cost, sims, cg, solves, inadmissible)."""
    out = dict(status=0, cost=0.0, sims=g["sims"].copy(), cg=0, solves=0, inadmissible=0)
    if not structure_ok(g):
        return dict(out, status=3)
    G = RefGraph(g)
    vals = np.concatenate([g["sims"].reshape(-1), g["meas"].reshape(-1)] + ([] if g.get("weight") is None else [g["weight"]]))
    bad = not np.isfinite(vals).all() or (g["sims"][:, 12] <= 0).any() or (g["meas"][:, 12] <= 0).any()
    bad = bad or (g.get("weight") is not None and (g["weight"] < 0).any())
    S = g["sims"].astype(F64)
    E, F, adm = G.evaluate(S)
    if bad or not adm:
        return dict(out, status=2)
    if G.ne == 0 or not G.free.any():
        return dict(out, status=1)
    iters, cg_iters, cg_tol, eps = prm
    lam, evals = LAMBDA_0, 1
    for _ in range(iters):
        out["solves"] += 1
        stats = dict(cg=0)
        ok, St, dmax = G.solve(S, E, lam, prm, stats)
        out["cg"] += stats["cg"]
        if not ok:
            lam = min(8.0 * lam, LAMBDA_MAX)
            continue
        Et, Ft, adm = G.evaluate(St)
        evals += 1
        if not adm:
            out["inadmissible"] += 1
            lam = min(8.0 * lam, LAMBDA_MAX)
            continue
        if Ft < F:
            S, E, F = St, Et, Ft
            lam = max(lam * 0.25, LAMBDA_MIN)
        else:
            lam = min(8.0 * lam, LAMBDA_MAX)
        if dmax <= eps:
            break
    return dict(out, status=evals << 8, cost=float(F), sims=S.astype(F32))


def ref_correct_points(so, sn, ref, xw):
    """(xw_out float32 [n][3], status uint8 [n])."""
    nv, n = len(so), len(xw)
    k = np.minimum(ref.astype(np.int64), max(nv - 1, 0))
    A, B = (so.astype(F64)[k], sn.astype(F64)[k]) if nv else (np.ones((n, 13)), np.ones((n, 13)))
    X = xw.astype(F64)
    with np.errstate(all="ignore"):
        c = [A[:, 12] * mat3(A[:, 3 * i], A[:, 3 * i + 1], A[:, 3 * i + 2], X[:, 0], X[:, 1], X[:, 2]) + A[:, 9 + i] for i in range(3)]
        d = [c[i] - B[:, 9 + i] for i in range(3)]
        Y = np.stack([(mat3(B[:, i], B[:, 3 + i], B[:, 6 + i], d[0], d[1], d[2]) / B[:, 12]).astype(F32) for i in range(3)], 1)
    ok = (ref.astype(np.int64) < nv) & np.isfinite(Y).all(1)
    return np.where(ok[:, None], Y, xw).astype(F32), (~ok).astype(np.uint8)


# ---- graphs -----------------------------------------------------------------------------------------------------------
def rot(v):
    v = np.asarray(v, F64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def sim(R, t, s):
    return np.concatenate([np.asarray(R, F64).reshape(-1), np.asarray(t, F64), [s]])


def sim_mul(A, B):
    Ra, Rb = A[:9].reshape(3, 3), B[:9].reshape(3, 3)
    return sim(Ra @ Rb, A[12] * Ra @ B[9:12] + A[9:12], A[12] * B[12])


def sim_inv(A):
    R = A[:9].reshape(3, 3)
    return sim(R.T, -(R.T @ A[9:12]) / A[12], 1.0 / A[12])


def rel(Si, Sj):
    """S_j o S_i^-1 in binary64."""
    return sim_mul(np.asarray(Sj, F64), sim_inv(np.asarray(Si, F64)))


def build_index(nv, edges):
    ne = len(edges)
    vert = np.asarray(edges, np.int64).reshape(-1)
    ent = np.arange(2 * ne)
    order = np.lexsort((ent, vert))
    ptr = np.zeros(nv + 1, np.uint32)
    ptr[1:] = np.cumsum(np.bincount(vert[vert < nv], minlength=nv)[:nv])
    return ptr, ent[order].astype(np.uint32)


def graph(sims, fixed, edges, meas, weight=None):
    sims = np.asarray(sims, F32).reshape(-1, 13)
    edges = np.asarray(edges, np.uint32).reshape(-1, 2)
    ptr, inc = build_index(len(sims), edges)
    return dict(sims=sims, fixed=np.asarray(fixed, np.uint8), edges=edges, meas=np.asarray(meas, F32).reshape(-1, 13),
                weight=None if weight is None else np.asarray(weight, F32), inc_ptr=ptr, inc=inc)


def trajectory(rng, n, fixed_scale=False, step=0.25):
    """n ground-truth similarities, world to camera, along a loose ring."""
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n
        R = rot([0.0, a, 0.0]) @ rot(rng.normal(0, 0.05, 3))
        c = np.array([4 * np.cos(a), 0.3 * rng.normal(), 4 * np.sin(a)])
        s = 1.0 if fixed_scale else float(np.exp(rng.normal(0, 0.05)))
        out.append(sim(R, -s * R @ c, s))
    return np.array(out)


def drifted(rng, truth, rot_sigma=0.004, t_sigma=0.02, s_sigma=0.004, fixed_scale=False):
    """The trajectory as odometry would give it: every relative motion perturbed, vertex 0 kept."""
    out = [truth[0]]
    for k in range(1, len(truth)):
        m = rel(truth[k - 1], truth[k])
        noise = sim(rot(rng.normal(0, rot_sigma, 3)), rng.normal(0, t_sigma, 3), 1.0 if fixed_scale else float(np.exp(rng.normal(0, s_sigma))))
        out.append(sim_mul(sim_mul(noise, m), out[-1]))
    return np.array(out)


def make_graph(seed, nv=12, extra=0, fixed=(0,), loops=((-1, 0),), weights=False, fixed_scale=False, drift=1.0, span=6):
    """A chain 0 - 1 - .. - nv-1 and `extra` covisibility edges measured from the drifted similarities (as ORB-SLAM takes
    them from the uncorrected poses), then loop edges measured from the ground truth, which the drift contradicts."""
    rng = np.random.default_rng(seed)
    truth = trajectory(rng, nv, fixed_scale)
    est = drifted(rng, truth, 0.004 * drift, 0.02 * drift, 0.004 * drift, fixed_scale).astype(F32)
    edges = [(k, k + 1) for k in range(nv - 1)]
    seen = set(edges)
    while len(edges) < nv - 1 + extra:
        i = int(rng.integers(0, nv))
        j = int(np.clip(i + rng.integers(2, span), 0, nv - 1))
        if i != j and (i, j) not in seen:
            edges.append((i, j)), seen.add((i, j))
    meas = [rel(est[i], est[j]) for i, j in edges]
    for i, j in loops:
        i, j = i % nv, j % nv
        edges.append((i, j))
        meas.append(rel(truth[i], truth[j]))
    fx = np.zeros(nv, np.uint8)
    fx[list(fixed)] = 1
    w = rng.uniform(0.25, 4.0, len(edges)).astype(F32) if weights else None
    return graph(est, fx, edges, meas, w)


def edit(g, **kw):
    out = {k: (None if v is None else v.copy()) for k, v in g.items()}
    out.update(kw)
    return out


def star(seed, leaves=300):
    """Vertex 0 (free) of degree `leaves`; leaf 1 is fixed."""
    rng = np.random.default_rng(seed)
    truth = trajectory(rng, leaves + 1)
    est = truth.copy()
    for k in range(leaves + 1):
        if k != 1:
            est[k] = sim_mul(sim(rot(rng.normal(0, 0.01, 3)), rng.normal(0, 0.05, 3), float(np.exp(rng.normal(0, 0.01)))), truth[k])
    edges = [(0, k) if k % 2 else (k, 0) for k in range(1, leaves + 1)]
    fx = np.zeros(leaves + 1, np.uint8)
    fx[1] = 1
    return graph(est, fx, edges, [rel(truth[i], truth[j]) for i, j in edges])


def two_vertices(seed):
    """The smallest graph: vertex 0 fixed, vertex 1 free, one edge whose measurement the similarities miss slightly."""
    rng = np.random.default_rng(seed)
    t = trajectory(rng, 2)
    off = sim(rot(rng.normal(0, 0.02, 3)), rng.normal(0, 0.1, 3), float(np.exp(rng.normal(0, 0.02))))
    return graph(t, [1, 0], [(0, 1)], [sim_mul(off, rel(t[0], t[1]))])


def pi_edge():
    """Two vertices at the identity and a measurement rotated by pi: 1 + tr R_E = 0 at the input state."""
    I = sim(np.eye(3), [0, 0, 0], 1.0)
    return graph([I, I], [1, 0], [(0, 1)], [sim(np.diag([-1.0, -1.0, 1.0]), [0, 0, 0], 1.0)])


def conflicting():
    """A free vertex (the j of both edges) between two fixed ones: one edge's error is a rotation of 177.5 degrees about
    z (admissible: 1 + tr = 0.0019), the other's of -5 degrees.  The first step is the mean of the two residuals, a
    rotation of about 175 degrees, which takes the second edge to about -180 degrees: an inadmissible trial state."""
    I = sim(np.eye(3), [0, 0, 0], 1.0)
    m = [sim(rot([0, 0, np.deg2rad(177.5)]), [0.05, -0.02, 0.01], 1.0), sim(rot([0, 0, np.deg2rad(-5.0)]), [0.0, 0.03, 0.0], 1.0)]
    return graph([I, I, I], [1, 0, 1], [(0, 1), (2, 1)], m)


SMALL = (6, 40, 1e-8, 1e-9)
BIG = (3, 12, 1e-3, 1e-9)


@functools.lru_cache(maxsize=None)
def cases():
    """(name, graph, parameters)."""
    out = []
    out.append(("two_vertices_one_edge", two_vertices(1), DEFAULT))
    out.append(("chain_of_3_middle_fixed", make_graph(2, nv=3, fixed=(1,), loops=((2, 0),)), DEFAULT))
    out.append(("ring_12_with_loop_edge", make_graph(3, nv=12, extra=6), DEFAULT))
    w = make_graph(4, nv=10, extra=5, weights=True)
    w["weight"][3] = 0.0
    out.append(("weights_with_a_zero", w, DEFAULT))
    out.append(("star_degree_300", star(5), BIG))
    out.append(("sparse_257", make_graph(6, nv=257, extra=120, drift=0.2), BIG))
    out.append(("sparse_1025", make_graph(7, nv=1025, extra=500, drift=0.05), BIG))
    out.append(("fixed_scale_like", make_graph(8, nv=12, extra=4, fixed_scale=True), DEFAULT))
    out.append(("two_fixed_vertices", make_graph(9, nv=9, extra=3, fixed=(0, 4)), SMALL))
    base = make_graph(10, nv=6, extra=2)
    ne = len(base["edges"])
    out.append(("code_1_no_edge", graph(base["sims"], base["fixed"], np.zeros((0, 2)), np.zeros((0, 13))), DEFAULT))
    out.append(("code_1_no_free_vertex", edit(base, fixed=np.ones(6, np.uint8)), DEFAULT))
    s = base["sims"].copy()
    s[2, 10] = np.nan
    out.append(("code_2_nan", edit(base, sims=s), DEFAULT))
    s = base["sims"].copy()
    s[3, 12] = 0.0
    out.append(("code_2_scale_not_positive", edit(base, sims=s), DEFAULT))
    m = base["meas"].copy()
    m[1, 12] = -1.0
    out.append(("code_2_measured_scale_negative", edit(base, meas=m), DEFAULT))
    wt = np.ones(ne, F32)
    wt[2] = -0.5
    out.append(("code_2_negative_weight", edit(base, weight=wt), DEFAULT))
    wt = np.ones(ne, F32)
    wt[0] = np.inf
    out.append(("code_2_infinite_weight", edit(base, weight=wt), DEFAULT))
    out.append(("code_2_edge_rotated_by_pi", pi_edge(), DEFAULT))
    e = base["edges"].copy()
    e[1, 1] = 6
    out.append(("code_3_bad_index", edit(base, edges=e), DEFAULT))
    e = base["edges"].copy()
    e[2, 1] = e[2, 0]
    ptr, inc = build_index(6, e)
    out.append(("code_3_i_equals_j", edit(base, edges=e, inc_ptr=ptr, inc=inc), DEFAULT))
    inc = base["inc"].copy()
    inc[0] ^= 1
    out.append(("code_3_entry_on_the_wrong_side", edit(base, inc=inc), DEFAULT))
    inc = base["inc"].copy()
    k = int(np.flatnonzero(np.diff(base["inc_ptr"].astype(np.int64)) >= 2)[0])
    a = int(base["inc_ptr"][k])
    inc[a], inc[a + 1] = inc[a + 1], inc[a]
    out.append(("code_3_unsorted_incidence", edit(base, inc=inc), DEFAULT))
    ptr = base["inc_ptr"].copy()
    ptr[6] -= 1
    out.append(("code_3_index_too_short", edit(base, inc_ptr=ptr), DEFAULT))
    out.append(("code_3_no_fixed_vertex", edit(base, fixed=np.zeros(6, np.uint8)), DEFAULT))
    lone = graph(np.concatenate([base["sims"], base["sims"][:1]]), np.concatenate([base["fixed"], [0]]), base["edges"], base["meas"])
    out.append(("free_vertex_without_an_edge", lone, SMALL))
    out.append(("trial_state_inadmissible", conflicting(), SMALL))
    return out


# ---- the host probe -------------------------------------------------------------------------------------------------
def hexf(a):
    return " ".join("%08x" % v for v in np.asarray(a, F32).reshape(-1).view(np.uint32))


def hexd(v):
    return "%016x" % int(np.array(v, F64).view(np.uint64))


def case_line(g, prm):
    nv, ne = len(g["sims"]), len(g["edges"])
    w = g.get("weight")
    parts = ["G %d %d %s %s %d %d %d" % (prm[0], prm[1], hexd(prm[2]), hexd(prm[3]), int(w is not None), nv, ne)]
    for k in range(nv):
        parts.append("%d %s" % (g["fixed"][k], hexf(g["sims"][k])))
    for e in range(ne):
        parts.append("%d %d %s %s" % (g["edges"][e][0], g["edges"][e][1], hexf(g["meas"][e]), hexf([1.0 if w is None else w[e]])))
    parts.append(" ".join(str(int(v)) for v in g["inc_ptr"]))
    parts.append(" ".join(str(int(v)) for v in g["inc"]))
    return " ".join(p for p in parts if p)


def points_line(so, sn, ref, xw):
    parts = ["P %d %d" % (len(so), len(xw)), hexf(so), hexf(sn)]
    parts += ["%d %s" % (ref[p], hexf(xw[p])) for p in range(len(xw))]
    return " ".join(p for p in parts if p)


@functools.lru_cache(maxsize=None)
def probe_exe():
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(tempfile.mkdtemp(prefix="graph_probe_"), "graph_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", "graph_host_check.cpp"), "-o", exe])
    return exe


def run_probe(lines):
    exe = probe_exe()
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        got = subprocess.run([exe, f.name], check=True, capture_output=True, text=True).stdout.splitlines()
    finally:
        os.unlink(f.name)
    assert len(got) == len(lines)
    return got


def probe(graphs, prms):
    """The probe's outputs for the graphs, as ref_graph's dicts."""
    out = []
    for g, ln in zip(graphs, run_probe([case_line(g, p) for g, p in zip(graphs, prms)])):
        t = ln.split()
        nv = len(g["sims"])
        assert len(t) == 4 + 13 * nv
        out.append(dict(status=int(t[0]), cost=float(np.array(int(t[1], 16), np.uint64).view(F64)), cg=int(t[2]), solves=int(t[3]),
                        sims=np.array([int(x, 16) for x in t[4:]], np.uint32).view(F32).reshape(nv, 13)))
    return out


def probe_points(so, sn, ref, xw):
    t = run_probe([points_line(so, sn, ref, xw)])[0].split()
    assert len(t) == 4 * len(xw)
    t = np.array(t).reshape(-1, 4)
    return (np.array([[int(x, 16) for x in row[1:]] for row in t], np.uint32).view(F32).reshape(-1, 3),
            np.array([int(x) for x in t[:, 0]], np.uint8))


def bits(a, dt=F32):
    return np.ascontiguousarray(np.asarray(a, dt)).view(np.uint32 if dt == F32 else np.uint64).reshape(-1).tolist()


def assert_same(got, want, tag):
    assert got["status"] == want["status"], (tag, got["status"], want["status"])
    assert bits(got["cost"], F64) == bits(want["cost"], F64), (tag, got["cost"], want["cost"])
    assert bits(got["sims"]) == bits(want["sims"]), tag
    if "cg" in got and "cg" in want:
        assert (got["cg"], got["solves"]) == (want["cg"], want["solves"]), tag


# ---- CPU tests --------------------------------------------------------------------------------------------------------
def test_pose_graph_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for f in ("pislam_pose_graph_batch", "pislam_pose_graph_reserve", "pislam_map_points_correct_batch"):
        assert re.search(r"\bint\s+%s\s*\(" % f, code), f
    m = re.search(r"typedef struct pislam_pose_graph_params \{([^}]*)\} pislam_pose_graph_params;", code)
    assert m, "pislam_pose_graph_params is not declared"
    fields = re.findall(r"(int32_t|double)\s+(\w+)\s*;", m.group(1))
    assert [f[1] for f in fields] == PG_FIELDS and [f[0] for f in fields] == ["int32_t"] * 2 + ["double"] * 2
    assert "#define PISLAM_ABI_VERSION 2" in text and "differs from g2o's Sim3 log in the terms of higher order" in text
    from pislam_amd import capi, frontend
    assert len(capi.SYMBOLS["pislam_pose_graph_batch"][1]) == 17 and len(capi.SYMBOLS["pislam_pose_graph_reserve"][1]) == 4
    assert len(capi.SYMBOLS["pislam_map_points_correct_batch"][1]) == 12
    assert [f[0] for f in capi.PoseGraphParams._fields_] == PG_FIELDS and ctypes.sizeof(capi.PoseGraphParams) == 24
    for f in ("essentialGraph", "reservePoseGraph", "poseGraphBatch", "correctMapPointsBatch", "rigidFromSim3"):
        assert callable(getattr(frontend, f))
    lib = capi.load()
    for f in ("pislam_pose_graph_batch", "pislam_pose_graph_reserve", "pislam_map_points_correct_batch"):
        assert hasattr(lib, f)
    assert "graph_host_check.cpp" in open(os.path.join(ROOT, "tools", "probes", "README.md")).read()


def test_pose_graph_probe_equals_the_restatement():
    cs = cases()
    got = probe([g for _, g, _ in cs], [p for _, _, p in cs])
    codes = set()
    for (name, g, prm), x in zip(cs, got):
        want = ref_graph(g, prm)
        assert_same(x, want, name)
        codes.add(want["status"] & 255)
        if name.startswith("code_"):
            assert want["status"] == int(name[5]) and want["cost"] == 0.0 and bits(want["sims"]) == bits(g["sims"]), name
        else:
            assert want["status"] & 255 == 0, name
        if name == "free_vertex_without_an_edge":            # every solve fails: the state is kept
            assert want["status"] == 1 << 8 and want["solves"] == prm[0] and bits(want["sims"]) == bits(g["sims"])
        elif name == "trial_state_inadmissible":
            assert want["inadmissible"] >= 1
        elif not name.startswith("code_"):                   # the graph moved and its cost fell
            assert want["status"] >> 8 >= 2 and bits(want["sims"]) != bits(g["sims"]), name
            assert want["cost"] < RefGraph(g).evaluate(g["sims"].astype(F64))[1], name
            fx = g["fixed"] != 0
            assert bits(want["sims"][fx]) == bits(g["sims"][fx]), name
    assert codes == {0, 1, 2, 3}


def random_edge(rng, norm):
    """(M, S_i, S_j) in binary64 with a residual of about `norm` (exactly 0 for norm == 0 up to rounding)."""
    Si = sim(rot(rng.normal(0, 1.0, 3)), rng.normal(0, 2.0, 3), float(np.exp(rng.normal(0, 0.3))))
    M = sim(rot(rng.normal(0, 1.0, 3)), rng.normal(0, 2.0, 3), float(np.exp(rng.normal(0, 0.3))))
    d = rng.normal(0, 1, 7)
    d *= norm / np.linalg.norm(d)
    Einv = sim_inv(ref_retract(sim(np.eye(3), [0, 0, 0], 1.0), d))   # E = the retraction of the identity by d: r = d
    Sj = sim_mul(Einv, sim_mul(M, Si))
    return M, Si, Sj


JAC_H = 2.0 ** -17
JAC_T = 32.0                                   # no translation word, and no entry of a differenced Jacobian, exceeds it
# What central differences with step h = 2^-17 resolve: a residual word is the end of about 64 rounded operations on
# words below T, so the difference of two of them over 2 h carries at most 64 * 2^-53 * T / h = 3.0e-8 of rounding; the
# truncation is h^2 / 6 times a third derivative, which for these rational functions of words below T stays below 64 T:
# 2.0e-8.  The bound is the sum of the two.
JAC_BOUND_0 = 64 * 2.0 ** -53 * JAC_T / JAC_H + JAC_H ** 2 / 6 * 64 * JAC_T
# Away from r = 0 the rotation and scale rows are first-order approximations: the deviation grows like |r|.  Measured
# worst relative deviations (largest |J - J_fd| over largest |J_fd|) over the 20 edges: 1.85e-4 at |r| = 1e-3 and 1.82e-2
# at |r| = 1e-1; a wrong sign or a missing term shows as a deviation of order 1.
JAC_MEASURED = {1e-3: 1.85e-4, 1e-1: 1.82e-2}


def jacobian_deviation(seed, norm):
    rng = np.random.default_rng(seed)
    M, Si, Sj = random_edge(rng, norm)
    E = ref_edge_error(M, Si, Sj)
    r, adm = ref_residual(E)
    assert adm and abs(np.linalg.norm(r) - norm) <= 1e-9 + 1e-6 * norm
    J = ref_jac(np.array([0, 1]), np.stack([E, E]), np.stack([M, M]))
    fd = np.zeros((2, 7, 7))
    for c in range(7):
        d = np.zeros(7)
        d[c] = JAC_H
        rp = ref_residual(ref_edge_error(M, ref_retract(Si, d), Sj))[0]
        rm = ref_residual(ref_edge_error(M, ref_retract(Si, -d), Sj))[0]
        fd[0, :, c] = (rp - rm) / (2 * JAC_H)
        rp = ref_residual(ref_edge_error(M, Si, ref_retract(Sj, d)))[0]
        rm = ref_residual(ref_edge_error(M, Si, ref_retract(Sj, -d)))[0]
        fd[1, :, c] = (rp - rm) / (2 * JAC_H)
    # the applied forms are the dense matrices
    p = rng.normal(0, 1, 7)
    for side, (fw, bw) in enumerate(((ref_ji(E, M, p), ref_jit(E, M, p)), (ref_jj(E, p), ref_jjt(E, p)))):
        assert np.abs(fw - J[side] @ p).max() <= 1e-13 * JAC_T and np.abs(bw - J[side].T @ p).max() <= 1e-13 * JAC_T
    assert max(np.abs(M[9:]).max(), np.abs(E[9:]).max(), np.abs(fd).max()) <= JAC_T
    return np.abs(J - fd).max(), np.abs(fd).max(), np.abs(J[:, 3:6] - fd[:, 3:6]).max()


def test_pose_graph_jacobians_against_central_differences():
    for seed in range(20):
        dev, _, _ = jacobian_deviation(100 + seed, 0.0)
        assert dev <= JAC_BOUND_0, (seed, dev)
    for norm, measured in JAC_MEASURED.items():
        worst = 0.0
        for seed in range(20):
            dev, scale, dev_t = jacobian_deviation(200 + seed, norm)
            worst = max(worst, dev / scale)
            assert dev_t <= JAC_BOUND_0, (seed, norm, dev_t)  # the translation rows are exact at any E
        print("jacobian deviation at |r| = %g: %.3g" % (norm, worst))
        assert worst <= 4 * measured, (norm, worst)


# ---- against a dense optimiser ----------------------------------------------------------------------------------------
def dense_lm(g, prm=DEFAULT, h=2.0 ** -20):
    """A binary64 Levenberg on the same residual with the same schedule: central-difference Jacobians of the restated
    residual under the restated retraction, the full damped normal equations through numpy.linalg.solve."""
    G = RefGraph(g)
    free = np.flatnonzero(G.free)
    col = {int(k): 7 * n for n, k in enumerate(free)}
    sw = np.sqrt(G.w)[:, None]

    def res(S):
        r, adm = ref_residual(ref_edge_error(G.M, S[G.i], S[G.j]))
        return (sw * r).reshape(-1), bool(adm.all())

    S = g["sims"].astype(F64)
    r, adm = res(S)
    assert adm
    F, lam = float(r @ r), LAMBDA_0
    iters, _, _, eps = prm
    for _ in range(iters):
        J = np.zeros((len(r), 7 * len(free)))
        for k in free:
            for c in range(7):
                d = np.zeros(7)
                d[c] = h
                Sp, Sm = S.copy(), S.copy()
                Sp[k], Sm[k] = ref_retract(S[k], d), ref_retract(S[k], -d)
                J[:, col[int(k)] + c] = (res(Sp)[0] - res(Sm)[0]) / (2 * h)
        A = J.T @ J
        A[np.diag_indices_from(A)] *= 1.0 + lam
        try:
            d = np.linalg.solve(A, -(J.T @ r)).reshape(-1, 7)
        except np.linalg.LinAlgError:
            lam = min(8.0 * lam, LAMBDA_MAX)
            continue
        St = S.copy()
        St[free] = ref_retract(S[free], d)
        rt, adm = res(St)
        Ft = float(rt @ rt)
        if adm and Ft < F:
            S, r, F, lam = St, rt, Ft, max(lam * 0.25, LAMBDA_MIN)
        else:
            lam = min(8.0 * lam, LAMBDA_MAX)
        if adm and np.abs(d).max() <= eps:
            break
    return S, F


DENSE_PRM = (20, 1024, 1e-12, 1e-9)            # enough conjugate-gradient iterations to converge every solve
DENSE_SEEDS = list(range(8))
# Measured over the 8 seeds (rings of 16 to 37 vertices): the call's final F deviates from the dense optimiser's by at
# most 9.70e-10 of it and no output word from the dense optimiser's by more than 1.42e-6 (the output is rounded to
# binary32: half an ulp of a word below 8 is 2.4e-7; the closed-form Jacobians are first-order in r, so the two stop at
# stationary points that differ in second order of the remaining residual).  The bounds are 8 times the measured
# values: 7.76e-9 and 1.14e-5.  The noise-free ring below ends within 4.77e-7 of its ground truth.
DENSE_COST_MEASURED, DENSE_POSE_MEASURED = 9.70e-10, 1.42e-6


@functools.lru_cache(maxsize=None)
def dense_graph(seed):
    nv = 16 + 3 * seed
    return make_graph(300 + seed, nv=nv, extra=nv // 2)


def dense_deviation(seed):
    g = dense_graph(seed)
    want = ref_graph(g, DENSE_PRM)
    S, F = dense_lm(g, DENSE_PRM)
    assert want["status"] & 255 == 0 and F < RefGraph(g).evaluate(g["sims"].astype(F64))[1] * 0.5
    return abs(want["cost"] - F) / F, float(np.abs(want["sims"].astype(F64) - S).max())


@pytest.mark.parametrize("seed", DENSE_SEEDS)
def test_pose_graph_against_a_dense_optimiser(seed):
    dc, dp = dense_deviation(seed)
    print("seed %d: cost deviation %.3g, pose deviation %.3g" % (seed, dc, dp))
    assert dc <= 8 * DENSE_COST_MEASURED and dp <= 8 * DENSE_POSE_MEASURED, (seed, dc, dp)


def exact_ring(seed, nv=24):
    """A noise-free ring: ground-truth similarities whose every word, and every word of every relative similarity, is
    exact in binary32 (axis permutations with signs, translations in eighths, scales that are powers of two), measured
    from the truth over chain, covisibility and loop edges; the start is the truth drifted, vertex 0 held."""
    rng = np.random.default_rng(seed)
    perms = [np.eye(3)[list(p)] * np.array(sg)[:, None] for p in ((0, 1, 2), (1, 2, 0), (2, 0, 1))
             for sg in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))]
    truth = np.array([sim(perms[int(rng.integers(0, len(perms)))], rng.integers(-32, 33, 3) / 8.0, 2.0 ** int(rng.integers(-1, 2)))
                      for _ in range(nv)])
    est = [truth[0]]
    for k in range(1, nv):
        noise = sim(rot(rng.normal(0, 0.004, 3)), rng.normal(0, 0.02, 3), float(np.exp(rng.normal(0, 0.004))))
        est.append(sim_mul(sim_mul(noise, rel(truth[k - 1], truth[k])), est[-1]))
    edges = [(k, k + 1) for k in range(nv - 1)] + [(k, k + 3) for k in range(0, nv - 3, 2)] + [(nv - 1, 0)]
    meas = np.array([rel(truth[i], truth[j]) for i, j in edges])
    assert (meas.astype(F32).astype(F64) == meas).all() and (truth.astype(F32).astype(F64) == truth).all()
    fx = np.zeros(nv, np.uint8)
    fx[0] = 1
    return graph(np.array(est), fx, edges, meas), truth


def test_pose_graph_noise_free_ring_reaches_the_ground_truth():
    for seed in range(4):
        g, truth = exact_ring(400 + seed)
        start = float(np.abs(g["sims"].astype(F64) - truth).max())
        want = ref_graph(g, DENSE_PRM)
        dev = float(np.abs(want["sims"].astype(F64) - truth).max())
        print("seed %d: start %.3g, end %.3g, cost %.3g" % (seed, start, dev, want["cost"]))
        assert want["status"] & 255 == 0 and start > 1e-2 and dev <= 8 * DENSE_POSE_MEASURED, (seed, start, dev)


# ---- map points moved with their key frames ---------------------------------------------------------------------------
def point_case(seed, nv=7, n=300):
    rng = np.random.default_rng(seed)
    so = trajectory(rng, nv).astype(F32)
    sn = np.array([sim_mul(sim(rot(rng.normal(0, 0.05, 3)), rng.normal(0, 0.3, 3), float(np.exp(rng.normal(0, 0.05)))), s)
                   for s in so.astype(F64)]).astype(F32)
    ref = rng.integers(0, nv, n).astype(np.uint16)
    xw = rng.uniform(-6, 6, (n, 3)).astype(F32)
    ref[5], ref[17], ref[n - 1] = nv, 0xFFFF, nv + 3         # out of range
    sn[2, 12] = 0.0                                          # a division by zero: not finite
    so[4, 9] = np.inf
    xw[40] = [np.nan, 1.0, 2.0]
    return so, sn, ref, xw


def test_map_points_correct_probe_equals_the_restatement():
    so, sn, ref, xw = point_case(500)
    want, st = ref_correct_points(so, sn, ref, xw)
    got, gst = probe_points(so, sn, ref, xw)
    assert gst.tolist() == st.tolist() and bits(got) == bits(want)
    bad = (ref >= len(so)) | (ref == 2) | (ref == 4)
    bad[40] = True
    assert st.tolist() == bad.astype(np.uint8).tolist() and bits(want[bad]) == bits(xw[bad])
    assert (want[~bad] != xw[~bad]).any(1).all()
    # no key frame at all: every point stays
    want0, st0 = ref_correct_points(so[:0], sn[:0], ref[:9], xw[:9])
    got0, gst0 = probe_points(so[:0], sn[:0], ref[:9], xw[:9])
    assert st0.tolist() == [1] * 9 == gst0.tolist() and bits(want0) == bits(xw[:9]) == bits(got0)


# ---- GPU tests --------------------------------------------------------------------------------------------------------
class Device:
    def __init__(self, ctx):
        import torch
        from pislam_amd import capi
        self.torch, self.capi, self.ctx, self.lib = torch, capi, ctx, ctx.lib

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda")

    def sentinels(self, B, V):
        t = self.torch
        f = lambda *s: t.full(s, SENT, dtype=t.int32, device="cuda")
        return dict(sims_out=f(B, V, 13).view(t.float32), cost=f(B, 2).view(t.float64).reshape(B), status=f(B))

    def pack(self, graphs, V, E, counts=None, weighted=None):
        """Host arrays of a batch: the slots at and beyond a graph's counts hold rubbish that must not be read.
        counts: per graph None or (v_counts, e_counts) as given to the call (may exceed the strides)."""
        B = len(graphs)
        rng = np.random.default_rng(7)
        weighted = any(g.get("weight") is not None for g in graphs) if weighted is None else weighted
        h = dict(sims=rng.normal(0, 1e30, (B, V, 13)).astype(F32), fixed=rng.integers(0, 256, (B, V)).astype(np.uint8),
                 edges=rng.integers(0, 1 << 32, (B, E, 2), dtype=np.uint64).astype(np.uint32),
                 meas=rng.normal(0, 1e30, (B, E, 13)).astype(F32),
                 weight=rng.normal(0, 1e30, (B, E)).astype(F32) if weighted else None,
                 inc_ptr=rng.integers(0, 1 << 32, (B, V + 1), dtype=np.uint64).astype(np.uint32),
                 inc=rng.integers(0, 1 << 32, (B, 2 * E), dtype=np.uint64).astype(np.uint32),
                 v_counts=np.zeros(B, np.uint32), e_counts=np.zeros(B, np.uint32))
        for b, g in enumerate(graphs):
            nv, ne = len(g["sims"]), len(g["edges"])
            h["sims"][b, :nv], h["fixed"][b, :nv], h["edges"][b, :ne], h["meas"][b, :ne] = g["sims"], g["fixed"], g["edges"], g["meas"]
            h["inc_ptr"][b, :nv + 1], h["inc"][b, :2 * ne] = g["inc_ptr"], g["inc"]
            if weighted:
                h["weight"][b, :ne] = 1.0 if g.get("weight") is None else g["weight"]
            c = (nv, ne) if counts is None or counts[b] is None else counts[b]
            h["v_counts"][b], h["e_counts"][b] = c
        for k in ("edges", "inc_ptr", "inc", "v_counts", "e_counts"):
            h[k] = h[k].view(np.int32)
        return h

    def upload(self, h):
        return {k: (None if v is None else self.up(v)) for k, v in h.items()}

    def call(self, prm, d, shape, B, o):
        ptr = self.capi.ptr
        p = None if prm is None else self.capi.PoseGraphParams(*prm)
        return self.lib.pislam_pose_graph_batch(
            self.ctx.h, None if p is None else ctypes.byref(p), ptr(d["sims"]), ptr(d["v_counts"]), ptr(d["fixed"]),
            ptr(d["edges"]), ptr(d["meas"]), ptr(d.get("weight")), ptr(d["e_counts"]), ptr(d["inc_ptr"]), ptr(d["inc"]),
            shape[0], shape[1], B, ptr(o["sims_out"]), ptr(o["cost"]), ptr(o["status"]))

    def run(self, graphs, prm, shape, counts=None, weighted=None):
        d = self.upload(self.pack(graphs, *shape, counts=counts, weighted=weighted))
        o = self.sentinels(len(graphs), shape[0])
        assert self.call(prm, d, shape, len(graphs), o) == 0, self.lib.pislam_last_error(self.ctx.h)
        self.ctx.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}


def assert_graphs(got, want, graphs, what=""):
    """Every output word of every graph, and the sentinels at and beyond the counts."""
    for b, (x, g) in enumerate(zip(want, graphs)):
        nv = len(g["sims"])
        assert_same(dict(status=int(got["status"][b]), cost=float(got["cost"][b]), sims=got["sims_out"][b, :nv]), x,
                    "%s graph %d" % (what, b))
        assert (got["sims_out"][b, nv:].view(np.uint32) == SENT).all(), (what, b)


def shape_of(graphs, pad=(0, 0)):
    return (max(max(len(g["sims"]) for g in graphs) + pad[0], 1), max(max(len(g["edges"]) for g in graphs) + pad[1], 1))


EMPTY = dict(sims=np.zeros((0, 13), F32), fixed=np.zeros(0, np.uint8), edges=np.zeros((0, 2), np.uint32),
             meas=np.zeros((0, 13), F32), weight=None, inc_ptr=np.zeros(1, np.uint32), inc=np.zeros(0, np.uint32))


@pytest.mark.gpu
def test_pose_graph_smallest_graph(gpu_ctx):
    g = two_vertices(11)
    want = ref_graph(g)
    assert want["status"] & 255 == 0 and bits(want["sims"]) != bits(g["sims"])
    got = Device(gpu_ctx).run([g], DEFAULT, (2, 1))
    assert_graphs(got, [want], [g], "smallest")


@pytest.mark.gpu
def test_pose_graph_every_case_in_batches_with_unequal_counts(gpu_ctx):
    """The graphs of the CPU test, one batch per parameter set, with padded strides, next to graphs whose counts are 0
    and PISLAM_COUNT_INVALID and one whose counts exceed the strides; once with weights (1.0 where a graph has none) and
    once, for the graphs without weights, with weight == NULL."""
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
            got = Device(gpu_ctx).run(batch, prm, (V + pad[0], E + pad[1]), counts if not any(pad) else counts[:-1] + [None],
                                      weighted=weighted)
            want = probe(batch, [prm] * len(batch))
            assert want[len(use)]["status"] == 3 and want[-1]["status"] & 255 == 0
            assert_graphs(got, want, batch, "%r weighted %r" % (prm, weighted))


@functools.lru_cache(maxsize=None)
def boundary_graphs():
    """255, 256 and 257 vertices (the partial count and the thread count), 1025 vertices, a vertex of degree 300."""
    gs = [make_graph(20 + n, nv=n, extra=n // 2, drift=0.2) for n in (255, 256, 257)]
    gs += [make_graph(24, nv=1025, extra=500, drift=0.05), star(25)]
    assert int(np.diff(gs[-1]["inc_ptr"].astype(np.int64)).max()) == 300
    return gs


@pytest.mark.gpu
def test_pose_graph_thread_and_partial_boundaries(gpu_ctx):
    gs = boundary_graphs()
    want = probe(gs, [BIG] * len(gs))
    assert all(x["status"] & 255 == 0 and x["status"] >> 8 >= 2 for x in want)
    got = Device(gpu_ctx).run(gs, BIG, shape_of(gs))
    assert_graphs(got, want, gs, "boundaries")


@pytest.mark.gpu
def test_pose_graph_at_the_limits(gpu_ctx):
    """One sparse graph of 4096 vertices and 16384 edges, few iterations."""
    g = make_graph(31, nv=MAX_V, extra=MAX_E - MAX_V, drift=0.01, span=40)
    assert shape_of([g]) == (MAX_V, MAX_E)
    prm = (2, 8, 1e-3, 1e-9)
    want = probe([g], [prm])
    assert want[0]["status"] == 3 << 8 and want[0]["cg"] == 16
    got = Device(gpu_ctx).run([g], prm, (MAX_V, MAX_E))
    assert_graphs(got, want, [g], "limits")


@pytest.mark.gpu
def test_pose_graph_second_pass_of_the_grid(gpu_ctx):
    """1026 two-vertex graphs: the second pass reuses the workspace slices of graphs that were refused and accepted."""
    gs = []
    for b in range(1026):
        g = two_vertices(1000 + b)
        if b % 5 == 1:
            g = edit(g, fixed=np.zeros(2, np.uint8))         # code 3
        elif b % 5 == 3:
            s = g["sims"].copy()
            s[1, b % 13] = np.nan
            g = edit(g, sims=s)                              # code 2
        gs.append(g)
    prm = (4, 8, 1e-6, 1e-9)
    want = probe(gs, [prm] * len(gs))
    assert {x["status"] & 255 for x in want} == {0, 2, 3} and want[1025]["status"] & 255 == 0 and want[1]["status"] == 3
    got = Device(gpu_ctx).run(gs, prm, (2, 1))
    assert_graphs(got, want, gs, "1026 graphs")


@pytest.mark.gpu
def test_pose_graph_in_place_and_refusals(gpu_ctx):
    d = Device(gpu_ctx)
    gs = [make_graph(41, nv=9, extra=4, weights=True), make_graph(42, nv=5, extra=1, weights=True)]
    V, E = shape = shape_of(gs, (2, 3))
    B = len(gs)
    h = d.pack(gs, *shape)
    dev = d.upload(h)
    o = d.sentinels(B, V)
    good = DEFAULT
    for prm in ((0, 256, 1e-6, 1e-9), (65, 256, 1e-6, 1e-9), (20, 0, 1e-6, 1e-9), (20, 1025, 1e-6, 1e-9), (20, 256, -1e-6, 1e-9),
                (20, 256, 1.0, 1e-9), (20, 256, float("nan"), 1e-9), (20, 256, 1e-6, -1e-9), (20, 256, 1e-6, float("nan")), None):
        assert d.call(prm, dev, shape, B, o) == -1, prm
    for bad in ((0, E), (MAX_V + 1, E), (V, 0), (V, MAX_E + 1)):
        assert d.call(good, dev, bad, B, o) == -1, bad
        assert d.lib.pislam_pose_graph_reserve(gpu_ctx.h, bad[0], bad[1], B) == -1, bad
    assert d.call(good, dev, shape, -1, o) == -1
    assert d.lib.pislam_pose_graph_reserve(gpu_ctx.h, V, E, -1) == -1
    host = np.zeros(B * (V + 1) * 13 + B * E * 13, np.int32)
    for name in ("sims", "v_counts", "fixed", "edges", "meas", "weight", "e_counts", "inc_ptr", "inc", "sims_out", "cost", "status"):
        for repl in (None, host):                             # NULL, then a host pointer
            if name == "weight" and repl is None:
                continue
            ins, outs = dict(dev), dict(o)
            (ins if name in ins else outs)[name] = repl
            assert d.call(good, ins, shape, B, outs) == -1, name
    # overlaps: an output on an input, two outputs on each other (partly, too)
    assert d.call(good, dev, shape, B, dict(o, status=dev["v_counts"])) == -1
    assert d.call(good, dev, shape, B, dict(o, sims_out=dev["meas"])) == -1
    assert d.call(good, dev, shape, B, dict(o, sims_out=dev["sims"].view(-1)[13:])) == -1
    assert d.call(good, dev, shape, B, dict(o, cost=o["sims_out"].view(-1).view(d.torch.float64))) == -1
    gpu_ctx.synchronize()
    for k, v in o.items():
        assert (v.cpu().numpy().view(np.uint8) == 0x5A).all(), k
    assert dev["sims"].cpu().numpy().tobytes() == h["sims"].tobytes()
    # batch 0 is a no-op after the checks: the pointers are not looked at
    p = d.capi.PoseGraphParams(*good)
    assert d.lib.pislam_pose_graph_batch(gpu_ctx.h, ctypes.byref(p), *([None] * 9), V, E, 0, None, None, None) == 0
    assert d.lib.pislam_pose_graph_reserve(gpu_ctx.h, V, E, 0) == 0
    # sims_out may be sims; nothing is written at or beyond the counts
    want = [ref_graph(g, good) for g in gs]
    assert all(x["status"] & 255 == 0 for x in want)
    assert d.call(good, dev, shape, B, dict(o, sims_out=dev["sims"])) == 0
    gpu_ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["sims_out"] = dev["sims"].cpu().numpy()
    for b, g in enumerate(gs):                                # beyond the counts the inputs' rubbish is untouched
        nv = len(g["sims"])
        assert got["sims_out"][b, nv:].tobytes() == h["sims"][b, nv:].tobytes()
        got["sims_out"][b, nv:].view(np.uint32)[...] = SENT
    assert_graphs(got, want, gs, "in place")


@pytest.mark.gpu
def test_pose_graph_determinism_and_graph_replay(gpu_ctx):
    """Two calls give the same bits; after pislam_pose_graph_reserve on a fresh context the call is captured on a side
    stream without a warm-up call, and both replays write what the eager call wrote."""
    import torch as t
    from pislam_amd.capi import Context
    from pislam_amd.frontend import poseGraphBatch, reservePoseGraph
    d = Device(gpu_ctx)
    gs = [make_graph(51, nv=20, extra=10), make_graph(52, nv=7, extra=2)]
    shape = shape_of(gs)
    dev = d.upload(d.pack(gs, *shape))
    args = (dev["sims"], dev["v_counts"], dev["fixed"], dev["edges"], dev["meas"], dev["weight"], dev["e_counts"], dev["inc_ptr"],
            dev["inc"])
    kw = dict(zip(PG_FIELDS, DEFAULT))
    first = [x.cpu().numpy().copy() for x in poseGraphBatch(*args, ctx=gpu_ctx, **kw, **d.sentinels(2, shape[0]))]
    again = [x.cpu().numpy().copy() for x in poseGraphBatch(*args, ctx=gpu_ctx, **kw, **d.sentinels(2, shape[0]))]
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    assert_graphs(dict(zip(("sims_out", "cost", "status"), first)), [ref_graph(g) for g in gs], gs, "frontend")
    gpu_ctx.synchronize()
    t.cuda.synchronize()
    side = t.cuda.Stream(t.device("cuda:0"))
    with t.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        reservePoseGraph(*shape, 2, ctx=ctx)
        o = d.sentinels(2, shape[0])
        side.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=side):
            poseGraphBatch(*args, ctx=ctx, **kw, **o)
        for _ in range(2):
            for x in o.values():
                x.view(t.uint8).fill_(0x5A)
            g.replay()
            side.synchronize()
            for a, b in zip(first, o.values()):
                assert a.tobytes() == b.cpu().numpy().tobytes()
        ctx.close()


@pytest.mark.gpu
def test_map_points_correct_grid_passes_in_place_and_bad_refs(gpu_ctx):
    """3 elements of 180000 points: 540000 threads' worth, which 1024 workgroups of 256 walk in three passes."""
    d = Device(gpu_ctx)
    t = d.torch
    B, P, V = 3, 180000, 9
    so, sn, ref, xw, cnt, vc = [], [], [], [], [P, P - 1234, COUNT_INVALID], [7, 9, 7]
    for b in range(B):
        a = point_case(600 + b, nv=7, n=P)
        pad = np.random.default_rng(b).normal(0, 1e30, (V - 7, 13)).astype(F32)
        so.append(np.concatenate([a[0], pad])), sn.append(np.concatenate([a[1], pad * 2])), ref.append(a[2]), xw.append(a[3])
    so, sn, ref, xw = np.stack(so), np.stack(sn), np.stack(ref), np.stack(xw)
    ref[1, ::97] = 8                                         # in range for element 1 alone (v_counts 9): rubbish similarities
    want, wst = xw.copy(), np.full((B, P), 0xA5, np.uint8)
    for b in range(B):
        n, nv = (0 if cnt[b] == COUNT_INVALID else min(cnt[b], P)), vc[b]
        want[b, :n], wst[b, :n] = ref_correct_points(so[b, :nv], sn[b, :nv], ref[b, :n], xw[b, :n])
    assert (wst[:2] == 0).sum() > 2 * P * 0.6 and (wst[:2] == 1).sum() > 1000
    ins = [d.up(x) for x in (xw, ref.view(np.int16), np.array(cnt, np.uint32).view(np.int32), so, sn, np.array(vc, np.int32))]
    ptr = d.capi.ptr
    call = lambda out, st, a=ins: d.lib.pislam_map_points_correct_batch(gpu_ctx.h, *[ptr(x) for x in a], P, V, B, ptr(out), ptr(st))
    out = t.full((B, P, 3), SENT, dtype=t.int32, device="cuda").view(t.float32)
    st = t.full((B, P), 0xA5, dtype=t.uint8, device="cuda")
    # refusals first: nothing is written
    assert d.lib.pislam_map_points_correct_batch(gpu_ctx.h, *[ptr(x) for x in ins], 0, V, B, ptr(out), ptr(st)) == -1
    assert d.lib.pislam_map_points_correct_batch(gpu_ctx.h, *[ptr(x) for x in ins], P, 0, B, ptr(out), ptr(st)) == -1
    assert d.lib.pislam_map_points_correct_batch(gpu_ctx.h, *[ptr(x) for x in ins], P, V, -1, ptr(out), ptr(st)) == -1
    for k in range(len(ins)):
        assert call(out, st, ins[:k] + [None] + ins[k + 1:]) == -1 and call(out, st, ins[:k] + [np.zeros(16, np.int32)] + ins[k + 1:]) == -1
    assert call(None, st) == -1 and call(out, None) == -1 and call(ins[3], st) == -1 and call(out, out.view(t.uint8)) == -1
    assert call(ins[0].view(-1)[3:], st) == -1
    gpu_ctx.synchronize()
    assert (out.view(t.int32) == SENT).all() and (st == 0xA5).all()
    assert call(out, st) == 0
    gpu_ctx.synchronize()
    got, gst = out.cpu().numpy(), st.cpu().numpy()
    assert gst.tobytes() == wst.tobytes()
    live = wst != 0xA5
    assert bits(got[live]) == bits(want[live]) and (got[~live].view(np.uint32) == SENT).all()
    # in place
    st.fill_(0xA5)
    assert call(ins[0], st) == 0
    gpu_ctx.synchronize()
    assert st.cpu().numpy().tobytes() == wst.tobytes() and bits(ins[0].cpu().numpy()) == bits(want)


@pytest.mark.gpu
def test_pose_graph_chain_to_corrected_points_and_poses(gpu_ctx):
    """similarities -> essentialGraph -> poseGraphBatch -> correctMapPointsBatch -> rigidFromSim3, with no conversion in
    between.  A point keeps its camera coordinates under its reference key frame's similarity, S_new(X') = S_old(X): the
    only rounding between the two sides is that of X' to binary32, at most 2^-24 |X'| a coordinate, which s R carries to
    at most s * 3 * 2^-24 * max|X'| a coordinate (0.8 <= s <= 1.25, |X'| <= 16 here: 3.6e-6).  Under the rigid poses (R,
    t / s) of rigidFromSim3 the camera coordinates are those divided by the scale, so they are kept up to the factor
    s_old / s_new (the map is rescaled with the key frame) and the pixel is kept; R is carried over exactly and t / s is
    rounded once, 2^-24 max|t / s| a side with |t / s| <= 16, the old side times s_old / s_new <= 1.5625: in all
    2^-24 * 16 * (3 + 1 + 1.5625) = 5.3e-6."""
    import torch as t
    from pislam_amd.frontend import correctMapPointsBatch, essentialGraph, poseGraphBatch, relativeSim3, rigidFromSim3
    d = Device(gpu_ctx)
    rng = np.random.default_rng(71)
    nv, npt = 16, 200
    truth = trajectory(rng, nv)
    est = drifted(rng, truth).astype(F32)
    pairs = [(k, k + 1) for k in range(nv - 1)] + [(k, k + 2) for k in range(0, nv - 2, 3)] + [(nv - 1, 0)]
    loop = rel(truth[nv - 1], truth[0]).astype(F32)[None]
    fixed = np.zeros(nv, np.uint8)
    fixed[0] = 1
    G = essentialGraph(d.up(est), d.up(fixed), d.up(np.array(pairs, np.int32)), meas=d.up(loop))
    sims, v_counts = G[0], G[1]
    # essentialGraph's arrays are what the restatement's own builders make of the same lists
    meas = [rel(est[i], est[j]) for i, j in pairs[:-1]] + [loop[0]]
    g = graph(est, fixed, pairs, meas)
    assert bits(G[4][0].cpu().numpy()) == bits(g["meas"]) and G[5] is None
    assert G[7][0].cpu().numpy().view(np.uint32).tolist() == g["inc_ptr"].tolist()
    assert G[8][0].cpu().numpy().view(np.uint32).tolist() == g["inc"].tolist()
    assert bits(relativeSim3(d.up(est[:1]), d.up(est[1:2])).cpu().numpy()) == bits(g["meas"][:1])
    sims_new, cost, status = poseGraphBatch(*G, ctx=gpu_ctx)
    gpu_ctx.synchronize()
    want = ref_graph(g)
    assert_same(dict(status=int(status[0]), cost=float(cost[0]), sims=sims_new[0].cpu().numpy()), want, "chain")
    assert want["status"] & 255 == 0 and want["cost"] < 0.05 * RefGraph(g).evaluate(est.astype(F64))[1]
    ref = rng.integers(0, nv, npt).astype(np.int16)
    xw = rng.uniform(-6, 6, (npt, 3)).astype(F32)
    xw2, st = correctMapPointsBatch(d.up(xw[None]), d.up(ref[None]), d.up(np.array([npt], np.int32)), sims, sims_new, v_counts,
                                    ctx=gpu_ctx)
    gpu_ctx.synchronize()
    assert int(st.sum()) == 0
    So, Sn, X2 = est.astype(F64)[ref], sims_new[0].cpu().numpy().astype(F64)[ref], xw2[0].cpu().numpy().astype(F64)
    moved = np.abs(Sn - So).max(1) > 1e-4
    assert moved.sum() > npt // 2 and np.abs(X2).max() <= 16
    assert min(Sn[:, 12].min(), So[:, 12].min()) >= 0.8 and max(Sn[:, 12].max(), So[:, 12].max()) <= 1.25
    cam = lambda S, X: S[:, 12:13] * np.einsum("nij,nj->ni", S[:, :9].reshape(-1, 3, 3), X) + S[:, 9:12]
    dev_sim = np.abs(cam(Sn, X2) - cam(So, xw.astype(F64)))[moved].max()
    print("similarity camera coordinates kept within %.3g" % dev_sim)
    assert dev_sim <= 1.25 * 3 * 2.0 ** -24 * 16
    Po, Pn = rigidFromSim3(sims[0]).cpu().numpy().astype(F64)[ref], rigidFromSim3(sims_new[0]).cpu().numpy().astype(F64)[ref]
    rigid = lambda P, X: np.einsum("nij,nj->ni", P[:, :9].reshape(-1, 3, 3), X) + P[:, 9:12]
    assert np.abs(Po[:, 9:]).max() <= 16 and np.abs(Pn[:, 9:]).max() <= 16
    a, b = rigid(Pn, X2), rigid(Po, xw.astype(F64)) * (So[:, 12:13] / Sn[:, 12:13])
    dev_rigid = np.abs(a - b)[moved].max()
    print("rigid camera coordinates kept, up to the scale, within %.3g" % dev_rigid)
    assert dev_rigid <= 2.0 ** -24 * 16 * (3 + 1 + 1.5625)
