"""Pins the float64 references of tests/decode_step_ref.py on the CPU: the prefix scorer against an enumeration of every alignment
(the only check of its semantics that does not go through the recursion), the float32 oracle against it on the chains the GPU file
runs (which measures how much of the tests' rounding bound a correct float32 implementation uses), the tie rule of topk_ref and the
float32 model of the fused scores against torch."""
import itertools
import math

import numpy as np
import pytest
import torch

from oracle.decoder import CTCPrefixScorer
from tests.decode_step_ref import (LOG_0, PREFIX_ROUNDINGS, CTCPrefixScorer64, attn_step_ref, beam_scores_ref, log_softmax_ref,
                                   lse_ref, prefix_bound, prefix_chain, prefix_emissions, topk_ref)
from tests.test_decode_step_kernels_gpu import PREFIX_CASES

BLANK, EOS = 0, 2


def _collapse(a):
    out, prev = [], -1
    for v in a:
        if v != prev and v != BLANK:
            out.append(v)
        prev = v
    return out


def _close(got, want):
    return abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_prefix_scorer_against_all_alignments(T):
    """V = 4: blank 0, <eos> 2, labels 1 and 3.  For every prefix h over the labels with |h| <= min(2, T) and every candidate c:
    exp(log_psi) = the summed probability of the alignments of all T frames whose collapsed sequence STARTS with h . c (c = <eos>:
    IS h; blank: 0), and exp(r[t]) = the probability that frames 0..t collapse to exactly h . c, split by whether frame t is blank
    (rows t >= start; below it the true probability is 0 = exp(LOG_0), but for the single-label sequence at t = 0)."""
    V = 4
    rs = np.random.RandomState(T)
    p = rs.dirichlet(np.ones(V), size=T)
    sc = CTCPrefixScorer64(np.log(p), BLANK, EOS)
    aligns = {n: [(a, float(np.prod([p[t, v] for t, v in enumerate(a)])), _collapse(a))
                  for a in itertools.product(range(V), repeat=n)] for n in range(1, T + 1)}
    state = {(): sc.initial_state()}
    prefixes = [()] + [(a,) for a in (1, 3)] + [(a, b) for a in (1, 3) for b in (1, 3)]
    checked = 0
    for h in prefixes:
        if len(h) > T:
            continue
        if h not in state:
            state[h] = sc([EOS] + list(h[:-1]), [h[-1]], state[h[:-1]])[1][0]
        cs = [1, 3, EOS, BLANK]
        log_psi, states = sc([EOS] + list(h), cs, state[h])
        start = max(len(h), 1)
        for j, c in enumerate(cs):
            g = list(h) + [c]
            if c == BLANK:
                assert log_psi[j] == LOG_0
                continue
            if c == EOS:
                want = sum(pa for a, pa, col in aligns[T] if col == list(h))
            else:
                want = sum(pa for a, pa, col in aligns[T] if col[:len(g)] == g)
            assert _close(math.exp(log_psi[j]), want), (h, c, math.exp(log_psi[j]), want)
            checked += 1
            if c == EOS:
                continue
            for t in range(T):
                for bl in (0, 1):
                    want = sum(pa for a, pa, col in aligns[t + 1] if col == g and (a[-1] == BLANK) == bool(bl))
                    if t >= start or (t == 0 and not h and bl == 0):
                        assert _close(math.exp(states[j, t, bl]), want), (h, c, t, bl)
                    else:
                        assert states[j, t, bl] == LOG_0 and want == 0.0, (h, c, t, bl)
    assert checked >= 3


def test_f32_oracle_stays_inside_the_rounding_bound_of_the_f64_scorer():
    """oracle/decoder.py::CTCPrefixScorer (float32) on the GPU file's cases, every call compared with the float64 scorer on the SAME
    previous state.  The bound is PREFIX_ROUNDINGS * n * 2^-24 * R (decode_step_ref.prefix_bound): per recursion step one logaddexp
    for phi, one for the state and one addition -- 3 roundings at the magnitude R of the state plus 8 at magnitude <= 1 inside the two
    logaddexp, <= 4 R for R >= 8.  Rows below start, blank and what the scorers copy are exact."""
    worst, worst_at = 0.0, None
    for T, V, nb in PREFIX_CASES:
        x = prefix_emissions(T, V, seed=T + V)
        sc32, sc64 = CTCPrefixScorer(x, BLANK, EOS), CTCPrefixScorer64(x, BLANK, EOS)
        r0 = sc32.initial_state()
        ref0 = sc64.initial_state()
        assert (r0[:, 0] == np.float32(LOG_0)).all() and r0[0, 1] == x[0, BLANK]
        assert (np.abs(r0[:, 1] - ref0[:, 1]) <= np.arange(T) * 2.0 ** -24 * np.abs(ref0[:, 1])).all()
        prev = None
        for st in prefix_chain(T, V, nb):
            cur = []
            for m in range(nb):
                r_prev = r0 if prev is None else prev[st.parent[m]][st.pcand[m]]
                psi32, s32 = sc32(st.hyps[m], st.cands[m], r_prev)
                psi64, s64 = sc64(st.hyps[m], st.cands[m], r_prev.astype(np.float64))
                assert psi32.dtype == np.float32 and s32.dtype == np.float32
                b_psi, b_st = prefix_bound(psi64, s64, r_prev, st.out_len, st.cands[m], EOS, BLANK)
                for got, ref, bound in ((psi32, psi64, b_psi), (s32, s64, b_st)):
                    err = np.abs(got.astype(np.float64) - ref)
                    assert (err[bound == 0] == 0).all(), (T, V, nb, st.out_len, m)
                    share = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
                    if share > worst:
                        worst, worst_at = share, (T, V, nb, st.out_len, m)
                cur.append(s32)
            prev = cur
    print(f"[measured] f32 oracle against the f64 prefix scorer: worst share of the bound {worst:.3f} at (T, V, nb, out_len, row) "
          f"{worst_at}; multiplier {PREFIX_ROUNDINGS}")
    assert worst <= 1.0, (worst, worst_at)      # PREFIX_ROUNDINGS = 4 roundings per step, counted above


def test_prefix_chain_reaches_the_edges():
    """the chains hold what the GPU test relies on: out_len 0..5, out_len == T, a parent used twice, both repeats and new tokens
    extended, every kind of candidate in every row"""
    for T, V, nb in PREFIX_CASES:
        chain = prefix_chain(T, V, nb)
        assert [s.out_len for s in chain] == list(range(min(6, T + 1)))
        for s in chain:
            assert all(len(h) - 1 == s.out_len for h in s.hyps)
            for m in range(nb):
                row = list(s.cands[m])
                assert EOS in row and BLANK in row and int(s.last[m]) in row and max(row.count(v) for v in row) >= 2
                assert all(0 <= v < V for v in row)
            if s.parent is not None and nb > 1:
                assert len(set(s.parent.tolist())) == nb - 1
    assert any(s.out_len == T for T, V, nb in PREFIX_CASES for s in prefix_chain(T, V, nb) if T >= 5)
    assert any(len(h) > 2 and h[-1] == h[-2] for T, V, nb in PREFIX_CASES for s in prefix_chain(T, V, nb) for h in s.hyps)


def test_topk_ref_tie_rule():
    s = np.array([[1.0, 3.0, 3.0, 0.5, 3.0, 2.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                  [-np.inf, 2.0, -np.inf, 2.0, 1.0, 2.0]])
    assert topk_ref(s, 4).tolist() == [[1, 2, 4, 5], [0, 1, 2, 3], [1, 3, 5, 4]]
    assert topk_ref(s, 2).tolist() == [[1, 2], [0, 1], [1, 3]]          # the boundary cuts the group of ties: the lowest indices stay
    assert topk_ref(s[0], 6).tolist() == [1, 2, 4, 5, 0, 3]


@pytest.mark.parametrize("V", [2, 257, 5000])
def test_beam_scores_ref_against_torch(V):
    g = torch.Generator().manual_seed(V)
    dec, lm = torch.randn(4, V, generator=g) * 3, torch.randn(4, V, generator=g) * 2
    dec[1] *= 25
    mu = float(np.float32(0.3))
    want = torch.log_softmax(dec.double(), -1) + mu * torch.log_softmax(lm.double(), -1)
    s, llm = beam_scores_ref(dec.numpy(), lm.numpy(), mu)
    assert s.dtype == np.float64 and np.abs(s - want.numpy()).max() <= 1e-12 * np.abs(want.numpy()).max()
    assert np.abs(llm - torch.log_softmax(lm.double(), -1).numpy()).max() <= 1e-12 * np.abs(llm).max()
    s32, llm32 = beam_scores_ref(dec.numpy(), lm.numpy(), mu, dtype=np.float32)
    assert s32.dtype == np.float32 and llm32.dtype == np.float32
    t32 = torch.log_softmax(dec, -1) + np.float32(mu) * torch.log_softmax(lm, -1)
    # two float32 evaluations with tree sums: log2(V) + 8 roundings each, at the magnitudes the values pass through
    u = (math.log2(V) + 8) * 2.0 ** -24
    mag = 2 + np.abs(lse_ref(dec.numpy()))[:, None] + np.abs(log_softmax_ref(dec.numpy())) \
        + mu * (np.abs(lse_ref(lm.numpy()))[:, None] + np.abs(llm)) + np.abs(s)
    assert (np.abs(s32.astype(np.float64) - t32.double().numpy()) <= 2 * u * mag).all()
    none, no_lm = beam_scores_ref(dec.numpy(), None, mu)
    assert no_lm is None and np.array_equal(none, log_softmax_ref(dec.numpy()))
    add = torch.randn(4, V + 3, generator=g).numpy()
    assert np.array_equal(log_softmax_ref(dec.numpy(), add=add, mu=mu), log_softmax_ref(dec.numpy()) + mu * add[:, :V].astype(np.float64))


def test_attn_step_ref_against_torch():
    g = torch.Generator().manual_seed(3)
    nb, d, H, Lmax, pos = 2, 32, 4, 9, 5
    qkv, kc, vc = torch.randn(nb, 3 * d, generator=g).double(), torch.randn(nb, Lmax, d, generator=g).double(), \
        torch.randn(nb, Lmax, d, generator=g).double()
    out, k2, v2 = attn_step_ref(qkv.numpy(), kc.numpy(), vc.numpy(), pos, H)
    kc[:, pos], vc[:, pos] = qkv[:, d:2 * d], qkv[:, 2 * d:]
    assert np.array_equal(k2, kc.numpy()) and np.array_equal(v2, vc.numpy())
    q = qkv[:, :d].view(nb, H, 1, d // H)
    k = kc[:, :pos + 1].view(nb, pos + 1, H, d // H).transpose(1, 2)
    v = vc[:, :pos + 1].view(nb, pos + 1, H, d // H).transpose(1, 2)
    want = (torch.softmax(q @ k.transpose(-1, -2) / (d // H) ** 0.5, -1) @ v).transpose(1, 2).reshape(nb, d)
    assert np.abs(out - want.numpy()).max() <= 1e-13
    out32, _, _ = attn_step_ref(qkv.numpy(), kc.numpy(), vc.numpy(), pos, H, dtype=np.float32)
    assert out32.dtype == np.float32 and np.abs(out32 - want.numpy()).max() <= 1e-5
