"""Vectorised restatement of the transducer loss (Graves 2012) for the kernel tests: the same quantities csrc/rnnt.hip produces
(lse / lpb / lpy per cell, alpha / beta over anti-diagonals, nll, the gradient w.r.t. the logits), in numpy.

dtype float64 is the REFERENCE (pinned against oracle/rnnt.py::rnnt_nll + autograd by tests/test_rnnt_ref_cpu.py).
dtype float32 is the model of a CORRECT f32 kernel: the same formulas in the same order -- m + log(1 + exp(-|a - b|)) for the lattice
sums, ((alpha + lp) + beta) + nll inside the occupancies, (exp(z - lse) * occ - gb - gy) * gs for the gradient -- evaluated in float32
with libm accuracy.  Its distance from the float64 result is the rounding a kernel cannot avoid; the tests scale their bounds by it.

TEST INFRASTRUCTURE ONLY."""
from collections import namedtuple

import numpy as np

RnntRef = namedtuple("RnntRef", "lse lpb lpy alpha beta nll dz valid gb gy")


def _lat_add(a, b):
    """log(exp(a) + exp(b)) as the lattice kernel forms it; -inf when both are -inf"""
    m = np.maximum(a, b)
    with np.errstate(invalid="ignore"):
        r = m + np.log(1 + np.exp(-np.abs(a - b)))
    return np.where(np.isneginf(m), m, r).astype(a.dtype)


def rnnt_ref(z, labels, elens, ylens, blank, gs=1.0, dtype=np.float64):
    """z [B,T,U,V] (any float array: cast to `dtype`), labels int [B,U-1], elens / ylens int [B]
    -> RnntRef of `dtype` arrays:
       lse, lpb, lpy [B,T,U]   every cell (lpy = -inf for u >= ylens[b])
       alpha, beta [B,T,U]     on `valid` (t < min(elens[b], T), u <= ylens[b]); -inf elsewhere
       nll [B]                 +inf for elens[b] <= 0
       dz [B,T,U,V]            gs * (softmax * occ - [v = blank] gb - [v = y] gy) on valid cells, 0 elsewhere and for nll = +inf
       gb, gy [B,T,U]          the occupancies of a cell's blank / label arc (occ = gb + gy, unscaled); 0 where dz is
       valid [B,T,U] bool"""
    z = np.asarray(z).astype(dtype)
    labels, elens, ylens = (np.asarray(a).astype(np.int64) for a in (labels, elens, ylens))
    B, T, U, V = z.shape
    gs = dtype(gs)
    ninf = dtype(-np.inf)
    m = z.max(-1)
    lse = (m + np.log(np.exp(z - m[..., None]).sum(-1, dtype=dtype))).astype(dtype)
    lpb = z[..., blank] - lse
    lpy = np.full((B, T, U), ninf, dtype)
    if U > 1:
        lab = np.broadcast_to(labels[:, None, :, None], (B, T, U - 1, 1))
        zy = np.take_along_axis(z[:, :, :U - 1], lab, -1)[..., 0] - lse[:, :, :U - 1]
        lpy[:, :, :U - 1] = np.where(np.arange(U - 1)[None, None, :] < ylens[:, None, None], zy, ninf)
    alpha = np.full((B, T, U), ninf, dtype)
    beta = np.full((B, T, U), ninf, dtype)
    nll = np.full(B, np.inf, dtype)
    valid = np.zeros((B, T, U), bool)
    dz = np.zeros((B, T, U, V), dtype)
    gbs, gys = np.zeros((B, T, U), dtype), np.zeros((B, T, U), dtype)
    for b in range(B):
        Tb, Ub = int(min(elens[b], T)), int(ylens[b])
        if Tb <= 0:
            continue
        valid[b, :Tb, :Ub + 1] = True
        pb, py = lpb[b], lpy[b]
        # one row / column of -inf around the lattice: the neighbours outside it drop out of the sums
        al = np.full((Tb + 1, Ub + 2), ninf, dtype)    # al[t + 1, u + 1] = alpha[t, u]
        be = np.full((Tb + 1, Ub + 2), ninf, dtype)    # be[t, u]         = beta[t, u]
        al[1, 1] = 0
        be[Tb - 1, Ub] = pb[Tb - 1, Ub]
        for d in range(1, Tb + Ub):
            u = np.arange(max(0, d - Tb + 1), min(Ub, d) + 1)
            t = d - u
            stay = al[t, u + 1] + np.where(t > 0, pb[t - 1, u], ninf)
            emit = al[t + 1, u] + np.where(u > 0, py[t, u - 1], ninf)
            al[t + 1, u + 1] = _lat_add(stay, emit)
            # the same diagonal counted from the far corner
            t, u = Tb - 1 - t, Ub - u
            stay = be[t + 1, u] + pb[t, u]
            emit = be[t, u + 1] + py[t, u]
            be[t, u] = _lat_add(stay, emit)
        alpha[b, :Tb, :Ub + 1] = al[1:, 1:]
        beta[b, :Tb, :Ub + 1] = be[:Tb, :Ub + 1]
        nl = -(al[Tb, Ub + 1] + pb[Tb - 1, Ub])
        nll[b] = nl
        if not np.isfinite(nl):
            continue
        a = al[1:, 1:]
        with np.errstate(over="ignore"):
            gb = np.exp(a + pb[:Tb, :Ub + 1] + be[1:, :Ub + 1] + nl)           # be[Tb] = -inf: no blank below the last frame ...
            gb[Tb - 1, Ub] = np.exp(a[Tb - 1, Ub] + pb[Tb - 1, Ub] + nl)       # ... except the one that ends the path
            gy = np.exp(a + py[:Tb, :Ub + 1] + be[:Tb, 1:] + nl)               # py = -inf at u = Ub
        occ = gb + gy
        gbs[b, :Tb, :Ub + 1], gys[b, :Tb, :Ub + 1] = gb, gy
        g = np.exp(z[b, :Tb, :Ub + 1] - lse[b, :Tb, :Ub + 1, None]) * occ[..., None]
        g[..., blank] -= gb
        if Ub > 0:
            tt, uu = np.meshgrid(np.arange(Tb), np.arange(Ub), indexing="ij")
            g[tt, uu, labels[b, :Ub][None, :]] -= gy[:, :Ub]
        dz[b, :Tb, :Ub + 1] = g * gs
    return RnntRef(lse, lpb, lpy, alpha, beta, nll, dz, valid, gbs, gys)
