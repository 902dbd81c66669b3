"""Numpy restatement of the CTC loss (Graves 2006) and of the two cross-entropy losses for the kernel tests: the quantities
csrc/ctc.hip produces (lse per row, the gathered emissions lp, alpha / beta over the extended label sequence, nll, the gradient
w.r.t. the logits, the greedy hypothesis) and the rows of csrc/decoder.hip::lsm_loss and csrc/distill.hip::soft_ce.

dtype float64 is the REFERENCE (pinned by tests/test_ctc_ref_cpu.py against path enumeration, torch's CTC on float64 CPU tensors
and autograd of a log_softmax restatement).
dtype float32 is the model of a CORRECT f32 kernel: the same formulas in the kernels' order -- m + log(exp(a - m) + exp(b - m) +
exp(c - m)) for the lattice sums, ((alpha + beta) - lp) + nll inside the occupancies, (exp(z - lse) - occupancies) * gs for the
gradient, -w * ((1 - eps) * lpy + off * (sum z - V * lse - lpy)) for the smoothed row -- evaluated in float32 with libm accuracy.
Its distance from the float64 result is the rounding a kernel cannot avoid; the tests scale their bounds by it.

TEST INFRASTRUCTURE ONLY."""
from collections import namedtuple

import numpy as np

CtcRef = namedtuple("CtcRef", "lse lp alpha beta nll dz valid")
CeRef = namedtuple("CeRef", "loss grad mag")


def _lat_add3(a, b, c):
    """log(exp(a) + exp(b) + exp(c)) as the lattice kernel forms it; -inf when all three are"""
    m = np.maximum(a, np.maximum(b, c))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = m + np.log(np.exp(a - m) + np.exp(b - m) + np.exp(c - m))
    return np.where(np.isneginf(m), m, r).astype(a.dtype)


def _log_add(a, b):
    """the pair sum that closes the lattice (common.h::log_add): m + log1p(exp(-|a - b|))"""
    if np.isneginf(a):
        return b
    if np.isneginf(b):
        return a
    return max(a, b) + np.log1p(np.exp(-abs(a - b)))


def _row_lse(z, dtype):
    m = z.max(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (m + np.log(np.exp(z - m[..., None]).sum(-1, dtype=dtype))).astype(dtype)


def ctc_ref(z, labels, elens, ylens, blank, gs=1.0, dtype=np.float64, row_scale=None):
    """z [B,T,V] (any float array: cast to `dtype`), labels int [B,Lmax], elens / ylens int [B] -> CtcRef of `dtype` arrays, with
    S = 2 * Lmax + 1 states (blank, y1, blank, ..., blank) and Sb = 2 * ylens[b] + 1 of them in use:
       lse [B,T]
       lp, alpha, beta [B,T,S]  on `valid` (t < min(elens[b], T), s < Sb); -inf elsewhere
       nll [B]                  +inf when no alignment exists or elens[b] == 0 < ylens[b]; 0 when both are 0
       dz [B,T,V]               gs * row_scale[b] * (softmax - occupancy); exactly 0 for t >= elens[b] and for a non-finite nll
                                (nn.CTCLoss(zero_infinity=True))
       valid [B,T,S] bool"""
    z = np.asarray(z).astype(dtype)
    labels, elens, ylens = (np.asarray(a).astype(np.int64) for a in (labels, elens, ylens))
    B, T, V = z.shape
    Lmax = labels.shape[1] if labels.ndim == 2 else 0
    S = 2 * Lmax + 1
    ninf = dtype(-np.inf)
    lse = _row_lse(z, dtype)
    lp = np.full((B, T, S), ninf, dtype)
    alpha = np.full((B, T, S), ninf, dtype)
    beta = np.full((B, T, S), ninf, dtype)
    nll = np.full(B, np.inf, dtype)
    valid = np.zeros((B, T, S), bool)
    dz = np.zeros((B, T, V), dtype)
    for b in range(B):
        Tb, L = int(min(elens[b], T)), int(ylens[b])
        Sb = 2 * L + 1
        if Tb <= 0:
            nll[b] = 0 if L == 0 else np.inf
            continue
        valid[b, :Tb, :Sb] = True
        ext = np.full(Sb, blank, np.int64)
        ext[1::2] = labels[b, :L]
        e = z[b, :Tb][:, ext] - lse[b, :Tb, None]                  # [Tb, Sb]
        lp[b, :Tb, :Sb] = e
        # may state s be entered from s - 2 (forward) / s + 2 (backward): a label whose neighbour label differs
        skip_f = np.zeros(Sb, bool)
        skip_b = np.zeros(Sb, bool)
        if L > 1:
            diff = labels[b, 1:L] != labels[b, :L - 1]
            skip_f[3::2] = diff
            skip_b[1:Sb - 2:2] = diff
        al = np.full((Tb, Sb + 2), ninf, dtype)                    # al[t, s + 2] = alpha[t, s]
        be = np.full((Tb, Sb + 2), ninf, dtype)                    # be[t, s]     = beta[t, s]
        al[0, 2:4] = e[0, :2]
        be[Tb - 1, max(Sb - 2, 0):Sb] = e[Tb - 1, max(Sb - 2, 0):]
        for t in range(1, Tb):
            p = al[t - 1]
            al[t, 2:] = _lat_add3(p[2:], p[1:-1], np.where(skip_f, p[:-2], ninf)) + e[t]
            q = be[Tb - t]
            be[Tb - 1 - t, :Sb] = _lat_add3(q[:Sb], q[1:Sb + 1], np.where(skip_b, q[2:], ninf)) + e[Tb - 1 - t]
        a, bt = al[:, 2:], be[:, :Sb]
        alpha[b, :Tb, :Sb], beta[b, :Tb, :Sb] = a, bt
        nl = dtype(-_log_add(a[Tb - 1, Sb - 1], a[Tb - 1, Sb - 2] if Sb >= 2 else ninf))
        nll[b] = nl
        if not np.isfinite(nl):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            occ = np.exp(((a + bt) - e) + nl)
        occ = np.where(np.isfinite(occ), occ, 0).astype(dtype)     # (an emission of -inf: no path through the state)
        with np.errstate(invalid="ignore"):
            g = np.exp(z[b, :Tb] - lse[b, :Tb, None]).astype(dtype)
        np.subtract.at(g, (np.arange(Tb)[:, None], ext[None, :]), occ)
        scale = dtype(gs) if row_scale is None else dtype(gs) * dtype(row_scale[b])
        dz[b, :Tb] = g * scale
    return CtcRef(lse, lp, alpha, beta, nll, dz, valid)


def ctc_greedy_ref(z, elens, blank):
    """z [B,T,V] -> (best int [B,T]: the row arg-max, first maximum wins; hyps: per utterance the frames t < min(elens[b], T)
    with repeats collapsed, then blanks dropped)"""
    z = np.asarray(z, np.float64)
    B, T, V = z.shape
    best = z.argmax(-1)
    hyps = []
    for b in range(B):
        hyp, prev = [], -1
        for t in range(int(min(elens[b], T))):
            v = int(best[b, t])
            if v != prev and v != blank:
                hyp.append(v)
            prev = v
        hyps.append(hyp)
    return best, hyps


def _smoothed(V, y, eps, dtype):
    off = dtype(eps) / dtype(V - 1)
    q = np.full(V, off, dtype)
    q[y] = dtype(1) - dtype(eps)
    return q, off


def lsm_ref(z, labels, w, eps, gs=1.0, dtype=np.float64):
    """label-smoothed cross-entropy rows (csrc/decoder.hip): q = 1 - eps on the label, eps / (V - 1) elsewhere
       loss[m] = -w[m] * sum_v q[v] log p[v];  grad[m, v] = gs * w[m] * (p[v] - q[v]);  mag[m] = |w[m]| * sum_v |q[v] log p[v]|
    (float64 always: the sum of the magnitudes of the terms the row is the sum of)"""
    z = np.asarray(z).astype(dtype)
    M, V = z.shape
    lse = _row_lse(z, dtype)
    loss, grad, mag = np.zeros(M, dtype), np.zeros((M, V), dtype), np.zeros(M)
    for m in range(M):
        wm, y = dtype(w[m]), int(labels[m])
        if wm == 0:
            continue
        q, off = _smoothed(V, y, eps, dtype)
        lpy = z[m, y] - lse[m]
        loss[m] = -wm * ((dtype(1) - dtype(eps)) * lpy + off * (z[m].sum(dtype=dtype) - dtype(V) * lse[m] - lpy))
        grad[m] = (dtype(gs) * wm) * (np.exp(z[m] - lse[m]) - q)
        z64 = z[m].astype(np.float64)
        mag[m] = abs(float(wm)) * np.abs(q.astype(np.float64) * (z64 - float(lse[m]))).sum()
    return CeRef(loss, grad, mag)


def soft_ce_ref(z, soft, src, hard, ws, wh, eps, gs=1.0, lrow=None, dtype=np.float64):
    """cross-entropy rows against a soft row + a smoothed hard label (csrc/distill.hip): row r reads z[lrow[r]] (r without lrow),
    q_s = soft[src[r]] (dropped for src[r] < 0), q_h = the smoothed one-hot of hard[r] (dropped for hard[r] < 0)
       loss[r]   = -(ws[r] * sum_v q_s[v] log p[v] + wh[r] * sum_v q_h[v] log p[v])
       grad[., v] = gs * (ws * (p[v] * sum(q_s) - q_s[v]) + wh * (p[v] - q_h[v]))      [M,V], zero on rows no r names
       mag[r]    = |ws| sum |q_s log p| + |wh| sum |q_h log p|   (float64)"""
    z = np.asarray(z).astype(dtype)
    M, V = z.shape
    rows = np.arange(M) if lrow is None else np.asarray(lrow).astype(np.int64)
    R = len(rows)
    lse = _row_lse(z, dtype)
    loss, grad, mag = np.zeros(R, dtype), np.zeros((M, V), dtype), np.zeros(R)
    g = dtype(gs)
    for r in range(R):
        lr = int(rows[r])
        sr = -1 if src is None else int(src[r])
        y = -1 if hard is None else int(hard[r])
        w_s = dtype(ws[r]) if sr >= 0 and ws is not None else dtype(0)
        w_h = dtype(wh[r]) if y >= 0 and wh is not None else dtype(0)
        if w_s == 0 and w_h == 0:
            continue
        x, l = z[lr], lse[lr]
        lp64 = x.astype(np.float64) - float(l)
        total, sq, minus = dtype(0), dtype(0), []
        if w_s != 0:
            q = np.asarray(soft[sr]).astype(dtype)
            sq = q.sum(dtype=dtype)
            total = total + w_s * ((q * x).sum(dtype=dtype) - l * sq)
            minus.append(g * w_s * q)
            mag[r] += abs(float(w_s)) * np.abs(q.astype(np.float64) * lp64).sum()
        if w_h != 0:
            qh, off = _smoothed(V, y, eps, dtype)
            lpy = x[y] - l
            total = total + w_h * ((dtype(1) - dtype(eps)) * lpy + off * (x.sum(dtype=dtype) - dtype(V) * l - lpy))
            minus.append(g * w_h * qh)
            mag[r] += abs(float(w_h)) * np.abs(qh.astype(np.float64) * lp64).sum()
        loss[r] = -total
        d = (g * (w_s * sq + w_h)) * np.exp(x - l)
        for term in minus:
            d = d - term
        grad[lr] = d
    return CeRef(loss, grad, mag)
