"""Reference for RNN-LM shallow fusion in the transducer beam search.  TEST INFRASTRUCTURE ONLY.

    search(scorer, lm_scorer, mu, T, W, E)   tests/rnnt_beam_ref.search (imported, not restated) over label tuples with the network's
                                             record replaced by the FUSED one: scorer(seq, t) -> lp f32 [V] (the joint's
                                             log-softmax row), lm_scorer(seq) -> lq f32 [V_lm >= V] (the LM's row after seq, <sos>
                                             first); candidates = the W best v >= 1 of f[v] = lp[v] + f32(mu) * lq[v] in f32 (product
                                             and sum rounded separately), ties to the lowest index; the blank extension is lp[blank];
                                             doubles from there on.  events.min_gap: the smallest score gap between neighbours at
                                             any cut of the search.
    finish(hyps, scores, len_weight)         final = score + len_weight * len(hyp) in doubles, stable descending re-sort
    hash_rows / hash_lm_rows                 the rows behind rnnt_beam_ref.hash_scorer (same hash, same generator) and LM rows in
                                             its style, keyed by the label sequence alone
"""
import zlib

import numpy as np

from tests import rnnt_beam_ref as R

BLANK, EOS = R.BLANK, R.EOS
GAP_TOL = 1e-4          # the bar between two forms of the search on the device (section 20): a case whose cuts are closer is left out


def hash_rows(seed, V, tie=False, scale=3.0):
    """scorer(seq, t) -> the f32 log-probability row of which rnnt_beam_ref.hash_scorer(seed, V, W, tie) returns the top W"""
    def scorer(seq, t):
        h = zlib.crc32(np.asarray([seed, t, len(seq)] + list(seq), dtype=np.int64).tobytes())
        x = np.random.default_rng(h).normal(size=V) * scale
        lp = x - np.logaddexp.reduce(x)
        if tie:
            lp = np.round(lp * 2.0) / 2.0
        return lp.astype(np.float32)
    return scorer


def hash_lm_rows(seed, V_lm, tie=False, scale=3.0):
    """lm_scorer(seq) -> f32 [V_lm]: a normalised row that depends on the label sequence alone (an LM does not see the frame)"""
    def lm_scorer(seq):
        h = zlib.crc32(np.asarray([seed, -1, len(seq)] + list(seq), dtype=np.int64).tobytes())
        x = np.random.default_rng(h).normal(size=V_lm) * scale
        lq = x - np.logaddexp.reduce(x)
        if tie:
            lq = np.round(lq * 2.0) / 2.0
        return lq.astype(np.float32)
    return lm_scorer


def fuse(lp, lq, mu, W):
    """-> (blank, vals[W], ids[W]): the record of emoasr_rnnt_beam_pick_lm for one row"""
    V = lp.shape[0]
    assert lq.shape[0] >= V and lp.dtype == np.float32 and lq.dtype == np.float32
    prod = np.float32(mu) * lq[1:V]                  # f32, rounded
    f = (lp[1:] + prod).astype(np.float32)           # f32, rounded again
    ids = np.argsort(-f, kind="stable")[:W]
    return np.float32(lp[BLANK]), f[ids].copy(), ids.astype(np.int64)


def fused_scorer(scorer, lm_scorer, mu, W):
    cache = {}

    def rec(seq, t):
        if seq not in cache:
            cache[seq] = lm_scorer(seq)
        return fuse(scorer(seq, t), cache[seq], mu, W)
    return rec


def search(scorer, lm_scorer, mu, T, W, E=3):
    """-> (hyps, scores, events), before the len_weight; rnnt_beam_ref.search asserts that grown candidates never fold"""
    return R.search(fused_scorer(scorer, lm_scorer, mu, W), T, W, E)


def finish(hyps, scores, len_weight):
    sc = [float(s) + float(len_weight) * float(len(h)) for h, s in zip(hyps, scores)]
    order = sorted(range(len(sc)), key=lambda i: -sc[i])
    return [hyps[i] for i in order], [sc[i] for i in order]


def oracle_scorers(sd, cfg, lm_sd, eouts):
    """(scorer, lm_scorer) of a real transducer (oracle.rnnt on the state dict sd) over encoder outputs eouts [1, T, d] and a real
    RNN LM (tests/rnnlm_ref on lm_sd), all f32 torch on the host: what min_gap of a golden-model search is read from"""
    import torch

    from oracle import rnnt as orn
    from tests import rnnlm_ref
    douts = {}

    def scorer(seq, t):
        if seq not in douts:
            douts[seq] = orn.recurrency(sd, cfg, torch.tensor([list(seq)]), None)[0][:, -1:]
        return torch.log_softmax(orn.joint(sd, eouts[:, t:t + 1], douts[seq])[0, 0, 0], -1).numpy().astype(np.float32)

    def lm_scorer(seq):
        lg = rnnlm_ref.logits(lm_sd, torch.tensor([list(seq)]))[0, -1]
        return torch.log_softmax(lg, -1).numpy().astype(np.float32)
    return scorer, lm_scorer


# (seed, V, V_lm, W, T, E, mu, len_weight): W in {1, 2, 4, 16}, T in {0, 1, 2, 12}, V - 1 == W and V - 1 > W, V_lm in {V, V + 3},
# E in {1, 3}.  The seeds are chosen so that this restatement alone meets the counts tests/test_rnnt_fusion_cpu.py asserts.
def _cases():
    out, s = [], 0
    for W in (1, 2, 4, 16):
        for T in (0, 1, 2, 12):
            for V in (W + 1, W + 4 if W < 16 else 40):
                out.append((300 + s, V, V + 3 * (s % 2), W, T, 3, (0.3, 1.0)[(s // 2) % 2], (0.5, 2.0)[s % 2]))
                s += 1
    for W, V in ((2, 5), (4, 9), (4, 40), (16, 40)):
        for T in (2, 12):
            out.append((300 + s, V, V + 3 * (s % 2), W, T, 1, 1.0, 1.0))
            s += 1
    for k in range(8):      # longer searches with room to disagree
        out.append((400 + k, 40, 40 + 3 * (k % 2), (4, 16)[k % 2], 12, 3, (1.0, 0.6)[k // 4], (0.7, 3.0)[k % 2]))
    return out


CASES = _cases()


def case_id(c):
    return "s%d-V%d-L%d-W%d-T%d-E%d-mu%g-len%g" % c


def scorers_of(case):
    seed, V, V_lm, W, T, E, mu, lw = case
    return hash_rows(seed, V), hash_lm_rows(seed + 5000, V_lm)
