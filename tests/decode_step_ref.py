"""Numpy restatement of the beam-search step kernels for the kernel tests: log_softmax, beam_scores_topk, topk, the CTC prefix
scorer (csrc/decoder.hip) and the single-query attention with cache append (csrc/rowlin.hip::attn_step).

dtype float64 is the REFERENCE (pinned by tests/test_decode_step_ref_cpu.py: the prefix scorer against an enumeration of all
alignments, the rest against torch on the CPU).
dtype float32 is the model of a CORRECT f32 kernel: the same formulas -- mx + log(sum exp(x - mx)), (x - lse) + mu * (lm - lse_lm),
softmax(q . K^T * scale) . V with the 1 / sum applied last -- evaluated in float32 with libm accuracy.  Its distance from the float64
result is the rounding a kernel cannot avoid; the tests scale their bounds by it (tests/ctc_ref.py does the same for the losses).

CTCPrefixScorer64 keeps the conventions of oracle/decoder.py::CTCPrefixScorer (LOG_0 = -1e10 for "log 0"; rows below
start = max(out_len, 1) are LOG_0, except r[0, 0] = x[0, c] for an empty prefix; <eos> scores logaddexp(r_prev[-1]); blank scores
LOG_0), but is written from the recursion of Watanabe et al., candidate by candidate in float64, not by casting the oracle.

prefix_chain builds the extension chains both test files run the scorers on.

TEST INFRASTRUCTURE ONLY."""
from collections import namedtuple

import numpy as np

LOG_0 = -1e10
LIVE = 1e9            # |value| below this: a log-probability; above: LOG_0 and what the recursion adds to it


# ---- log-softmax, fused scores, top-k ------------------------------------------------------------------------------------------------
def lse_ref(x, dtype=np.float64):
    """x [M,V] -> lse [M] of `dtype`: mx + log(sum exp(x - mx)); -inf entries count as probability 0"""
    x = np.asarray(x).astype(dtype)
    mx = x.max(-1)
    with np.errstate(divide="ignore"):
        return (mx + np.log(np.exp(x - mx[..., None]).sum(-1, dtype=dtype))).astype(dtype)


def log_softmax_ref(x, add=None, mu=0.0, dtype=np.float64):
    """out[m, v] = (x[m, v] - lse(x[m])) + mu * add[m, v]   ([M,V] of `dtype`; add: only its first V columns are read)"""
    x = np.asarray(x).astype(dtype)
    out = x - lse_ref(x, dtype)[..., None]
    if add is not None:
        out = out + dtype(mu) * np.asarray(add)[..., :x.shape[-1]].astype(dtype)
    return out.astype(dtype)


def beam_scores_ref(dec, lm, mu, dtype=np.float64):
    """-> (s, llm): llm = log_softmax(lm) (None without an LM), s = log_softmax(dec) + mu * llm"""
    s = log_softmax_ref(dec, dtype=dtype)
    if lm is None:
        return s, None
    llm = log_softmax_ref(lm, dtype=dtype)
    return (s + dtype(mu) * llm).astype(dtype), llm


def topk_ref(s, k):
    """indices [..., k] of the k largest of every row: value descending, index ascending among equals"""
    return np.argsort(-np.asarray(s), axis=-1, kind="stable")[..., :k]


# ---- CTC prefix scorer ---------------------------------------------------------------------------------------------------------------
class CTCPrefixScorer64:
    """x [T,V] log-probabilities.  State r [T,2]: r[t,0] / r[t,1] = log p(the prefix is emitted by frames 0..t, ending in its last
    label / in blank).  For a prefix h (y = [<sos>] + h, out_len = |h|), its state r_prev and a candidate c:
        phi[t]   = log p(h by frame t, in a way that c may follow at t + 1) = r_prev[t,1] if c repeats h's last label, else
                   logaddexp(r_prev[t,0], r_prev[t,1])
        r[t,0]   = logaddexp(r[t-1,0], phi[t-1]) + x[t,c]               (stay on c, or enter it)
        r[t,1]   = logaddexp(r[t-1,0], r[t-1,1]) + x[t,blank]
        log_psi  = log sum_t exp(phi[t-1] + x[t,c])  (+ x[0,c] for the empty prefix): c first emitted at t, anything after"""

    def __init__(self, x, blank_id, eos_id):
        self.x = np.asarray(x, np.float64)
        self.blank, self.eos, self.T = int(blank_id), int(eos_id), len(self.x)

    def initial_state(self):
        r = np.full((self.T, 2), LOG_0)
        r[:, 1] = np.cumsum(self.x[:, self.blank])
        return r

    def __call__(self, y, cs, r_prev):
        """-> (log_psi [C], states [C,T,2])"""
        r_prev = np.asarray(r_prev, np.float64)
        out_len, last, T = len(y) - 1, int(y[-1]), self.T
        start = max(out_len, 1)
        r_sum = np.logaddexp(r_prev[:, 0], r_prev[:, 1])
        xb = self.x[:, self.blank]
        log_psi = np.empty(len(cs))
        states = np.full((len(cs), T, 2), LOG_0)
        for j, c in enumerate(int(c) for c in cs):
            xc = self.x[:, c]
            phi = r_prev[:, 1] if out_len > 0 and c == last else r_sum
            r = states[j]
            if out_len == 0:
                r[0, 0] = xc[0]
            psi = r[start - 1, 0]
            for t in range(start, T):
                psi = np.logaddexp(psi, phi[t - 1] + xc[t])
                r[t, 0] = np.logaddexp(r[t - 1, 0], phi[t - 1]) + xc[t]
                r[t, 1] = np.logaddexp(r[t - 1, 0], r[t - 1, 1]) + xb[t]
            if c == self.eos:
                psi = r_sum[-1]
            if c == self.blank:
                psi = LOG_0
            log_psi[j] = psi
        return log_psi, states


# per recursion step in float32, in units of u = 2^-24 (one correctly rounded operation at magnitude 1), R the magnitude of the state:
#   phi = logaddexp(.,.)            1 R  (the final max + log1p)  + 4: the difference (<= 0.28: d e^-d / (1 + e^-d)), exp (1 ulp = 2 u
#                                        of a value <= 1) and log1p (2 u of a value <= 0.7) inside it
#   logaddexp(r, phi)               1 R + 4
#   + x[t]  (psi: phi + x[t])       1 R
# = 3 R + 8 <= 4 R for R >= 8; the blank recursion has one logaddexp fewer.  Errors of the operands pass through logaddexp with
# weights that sum to 1, so n steps give at most n times that.
PREFIX_ROUNDINGS = 4
PREFIX_R_FLOOR = 8.0


def prefix_bound(ref_psi, ref_states, r_prev, out_len, cs, eos, blank):
    """(bound_psi [C], bound_states [C,T,2]) = PREFIX_ROUNDINGS * n * 2^-24 * R per entry of one scorer call:
    n = the recursion steps behind the entry (t - start + 1 for row t, T - start for log_psi, 1 for <eos>, 0 -- exact -- for rows
    below start and for blank); R = max(8, the largest live magnitude among r_prev, the states and log_psi of the call), and the
    entry's own magnitude for entries at LOG_0 (whose float32 ulp is 1024)."""
    ref_psi, ref_states, r_prev = (np.asarray(a, np.float64) for a in (ref_psi, ref_states, r_prev))
    C, T, _ = ref_states.shape
    start = max(out_len, 1)
    live = [np.abs(a[np.abs(a) < LIVE]) for a in (ref_psi, ref_states, r_prev)]
    R = max([PREFIX_R_FLOOR] + [float(a.max()) for a in live if a.size])
    n_row = np.clip(np.arange(T) - start + 1, 0, None).astype(np.float64)[None, :, None]
    u = 2.0 ** -24
    b_states = PREFIX_ROUNDINGS * n_row * u * np.maximum(R, np.abs(ref_states))
    cs = np.asarray(cs)
    n_psi = np.where(cs == blank, 0.0, np.where(cs == eos, 1.0, float(max(T - start, 0))))
    b_psi = PREFIX_ROUNDINGS * n_psi * u * np.maximum(R, np.abs(ref_psi))
    return b_psi, b_states


PrefixStep = namedtuple("PrefixStep", "out_len hyps last cands parent pcand")


def prefix_emissions(T, V, seed):
    """f32 [T,V] log(dirichlet(0.5))"""
    rs = np.random.RandomState(seed)
    return np.log(rs.dirichlet(np.ones(V) * 0.5, size=T)).astype(np.float32)


def prefix_chain(T, V, nb, steps=6, cw=5, blank=0, eos=2, seed=0):
    """a chain of extension steps, out_len = 0, 1, ... (stopping where out_len would exceed T): nb rows of cw = 5 candidates each.
    Every candidate row holds, in random order: <eos>, blank, a repeat of the row's last token, a fresh token and that fresh token a
    second time (two candidates of one row that must come out equal).  From step 1 on row m extends candidate pcand[m] of row
    parent[m] of the step before -- parents permuted with one used twice, pcand one of the parent row's real tokens, rotating: its two
    fresh ones and, where the parent row is of step 1 or later, its repeat (at step 0 the row's last token is <eos>).
    -> [PrefixStep]; hyps include the leading <eos> (= <sos>), as the scorers take them."""
    assert cw == 5
    rs = np.random.RandomState(1000 * T + V + nb + seed)
    real = [v for v in range(V) if v not in (blank, eos)]
    out, prev = [], None
    for step in range(steps):
        if step > T:
            break
        if prev is None:
            hyps, parent, pcand = [[eos] for _ in range(nb)], None, None
        else:
            parent = rs.permutation(nb)
            if nb > 1:
                parent[-1] = parent[0]
            pcand = np.empty(nb, np.int64)
            hyps = []
            for m in range(nb):
                ok = [j for j in range(cw) if prev.cands[parent[m], j] not in (blank, eos)]
                pcand[m] = ok[(step + m) % len(ok)]
                hyps.append(prev.hyps[parent[m]] + [int(prev.cands[parent[m], pcand[m]])])
        last = np.array([h[-1] for h in hyps], np.int64)
        cands = np.empty((nb, cw), np.int64)
        for m in range(nb):
            fresh = int(rs.choice([v for v in real if v != last[m]]))
            cands[m] = rs.permutation([eos, blank, int(last[m]), fresh, fresh])
        prev = PrefixStep(step, hyps, last, cands, parent, pcand)
        out.append(prev)
    return out


# ---- single-query attention ----------------------------------------------------------------------------------------------------------
def attn_step_ref(qkv, kc, vc, pos, H, dtype=np.float64):
    """qkv [nb,3d] (q | k | v), kc / vc [nb,Lmax,d] -> (out [nb,d], kc', vc'): k and v are written to row pos of the caches, then
    out = softmax(q . K[:pos + 1]^T / sqrt(dk)) . V[:pos + 1] per head (dk = d / H), all in `dtype` (float32: scores, exponentials and
    the sum over positions accumulated position by position, the 1 / sum applied last)"""
    qkv, kc, vc = (np.asarray(a).astype(dtype) for a in (qkv, kc, vc))
    nb, d = qkv.shape[0], qkv.shape[1] // 3
    dk = d // H
    kc, vc = kc.copy(), vc.copy()
    kc[:, pos], vc[:, pos] = qkv[:, d:2 * d], qkv[:, 2 * d:]
    n = pos + 1
    q = qkv[:, :d].reshape(nb, H, dk)
    k = kc[:, :n].reshape(nb, n, H, dk)
    v = vc[:, :n].reshape(nb, n, H, dk)
    scale = dtype(1) / np.sqrt(dtype(dk))
    s = np.zeros((nb, n, H), dtype)
    for c in range(dk):
        s = s + q[:, None, :, c] * k[..., c]
    s = s * scale
    p = np.exp(s - s.max(1, keepdims=True)).astype(dtype)
    o = np.zeros((nb, H, dk), dtype)
    tot = np.zeros((nb, H), dtype)
    for t in range(n):
        o = o + p[:, t, :, None] * v[:, t]
        tot = tot + p[:, t]
    out = o * (dtype(1) / tot)[..., None]
    return out.reshape(nb, d).astype(dtype), kc, vc
