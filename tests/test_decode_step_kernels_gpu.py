"""The beam-search step kernels at kernel level: log_softmax, topk, beam_scores_topk, ctc_prefix_init / ctc_prefix_score and their
ragged twins (csrc/decoder.hip), emoasr_beam_cache_gather (csrc/decode_rt.hip) and attn_step (csrc/rowlin.hip) against the float64
references of tests/decode_step_ref.py (pinned on the CPU by tests/test_decode_step_ref_cpu.py), at the sizes where each kernel
changes path: the 256- and 1024-thread strides, the 4096-stride staging loop, candidates in registers / in LDS (V 16384 | 16385),
merge in registers / in LDS (k 32 | 33), the LM row in LDS / in global memory, the dynamic-LDS attribute (60 KiB) and the 150 KiB
limit, whole and partial 64-frame chunks of the prefix recursion with start = 1..5 and start == T, pos on both sides of the
64-position trips of attn_step, heads narrower and wider than a wave.

Bounds (none taken from the kernels under test; u = 2^-24, e32 = the distance of the float32 evaluation of the same formulas -- the
dtype=float32 of the references, the float32 oracle for the prefix scorer -- from the float64 reference on the same call):
  log-softmax values   |got - ref64| <= max(4 e32, (ceil(V / threads) + 16) u (1 + |lse| + |out|)), threads = 256
                       (log_softmax_kernel) or 1024 (beam_scores_topk_kernel), e32 per row.  Counted against the code: a term of the sum of
                       exponentials passes ceil(V / threads) - 1 additions in its thread, 6 wave levels and the sequential sum of
                       the waves' partials (3 | 15 more), after x - mx (1) and expf (1 ulp = 2 u): ceil + 11 | ceil + 23 roundings
                       of a relative error of se, an absolute one of log(se); then logf (2 u |log se|), mx + log(se) (u |lse|) and
                       x - lse (u |x - lse|).  The 256-thread kernel is covered in the worst case everywhere; the 1024-thread kernel
                       wherever 7 + 2 log(se) <= (ceil + 15) (|lse| + |x - lse|), i.e. |lse| + |x - lse| >= 1.8 -- below that only if
                       all of its 23 roundings fall the same way, and the margin is not widened for that corner.
                       The LM term of the fused scores: + |mu| times the same expression for the LM row.  (Derivation note: the
                       product mu * term and the final sum are two more instructions, u (|mu * term| + |out|), for the LM row and for
                       an `add` row alike; they are counted here and not added to the margin -- out is the final output.)
  top-k values         order statistics are 1-Lipschitz in the sup norm: vals[j] is within the row's largest bound of the j-th largest
                       float64 score; the float64 score at idx[j] is within that entry's bound of vals[j]
  prefix scorer        max(4 e32, 4 n u R) per entry, n = the recursion steps behind it, R = the magnitude of the state
                       (decode_step_ref.prefix_bound; the 4 is counted there and holds for the float32 oracle with share 0.24 on these
                       cases); every step is fed the device state of the step before, so the errors are per step.  No term for the
                       hardware exp / log had to be added (delta = 0): see the shares below.
  attn_step            2^-8 |ref| + 4 e32: one bf16 ulp of output rounding
  indices, rows below start, candidates given twice, untouched memory, gathered bytes, appended cache rows, ragged == dense: exact

MEASURED on an MI355X, worst share of the bound: log_softmax 0.05, with `add` 0.07 (f32 and bf16); beam_scores_topk values 0.05,
score at the returned index 0.06, lm_at 0.06 (all V, k, both dtypes, with and without the LM); prefix scorer 0.24 (an <eos> score:
one logaddexp, the same libm formula as the oracle, which also has 0.24), initial state 0.17, state rows behind 64 and more
recursion steps 0.03 of 4 n u R (the float32 oracle: the same 0.03) -- the hardware exp / log of the recursion does not show, the
error there is the additions' and grows more slowly than n, with no step at a chunk edge; attn_step 0.99 (the bf16 rounding of the
output, which is the bound's first term; the f32 model is 2e-7 .. 4e-7 off)."""
import math

import numpy as np
import pytest
import torch

from tests.decode_step_ref import (LIVE, LOG_0, PREFIX_ROUNDINGS, CTCPrefixScorer64, attn_step_ref, beam_scores_ref, log_softmax_ref,
                                   lse_ref, prefix_bound, prefix_chain, prefix_emissions, topk_ref)

pytestmark = pytest.mark.gpu

U24, P8 = 2.0 ** -24, 2.0 ** -8
NAN = float("nan")
MU = float(np.float32(0.3))          # (what the kernels receive: the weight is a C float)
BLANK, EOS = 0, 2
_DT = [torch.float32, torch.bfloat16]
_DT_IDS = ["f32", "bf16"]


def _i32(a, dev):
    return torch.as_tensor(np.asarray(a)).to(torch.int32).to(dev)


def _np64(t):
    return t.detach().double().cpu().numpy()


def _strided(z, dev, pad=5):
    """z [M,V] on the device as the [:, :V] view of a NaN-filled [M, V + pad] buffer"""
    M, V = z.shape
    wide = torch.full((M, V + pad), NAN, dtype=z.dtype)
    wide[:, :V] = z
    return wide.to(dev)[:, :V]


def _share(got, ref, bound):
    """-> (largest error, its largest share of the bound) over the entries where the reference is finite"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = np.broadcast_to(bound, ref.shape)
    ok = np.isfinite(ref)
    assert np.isfinite(got[ok]).all(), "non-finite value"
    err = np.abs(got[ok] - ref[ok])
    if err.size == 0:
        return 0.0, 0.0
    return float(err.max()), float((err / (bound[ok] + 1e-300)).max())


def _lsm_bound(x64, threads, out=None):
    """(ceil(V / threads) + 16) u (1 + |lse| + |out|) per entry of x64 [M,V], out = x - lse unless given; +inf where out is -inf
    (never compared)"""
    V = x64.shape[-1]
    lse = lse_ref(x64)[:, None]
    return (math.ceil(V / threads) + 16) * U24 * (1 + np.abs(lse) + np.abs(x64 - lse if out is None else out))


def _e32(m32, ref):
    """-> [M,1]: per row, the largest distance of the float32 model from the reference where the reference is finite"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(ref), np.abs(m32.astype(np.float64) - ref), 0).max(-1, keepdims=True)


# ---- log_softmax -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("V", [2, 255, 256, 257, 1000, 10000])
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_log_softmax(dev, dtype, V, with_add):
    """five rows of a strided view: three Gaussian rows, one scaled to reach +-80 (the max subtraction), one of equal values (exactly
    -log V up to the bound); `add` f32 with a row stride of its own, NaN behind the V columns"""
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(V)
    x = torch.randn(5, V, generator=g) * 2
    x[3] *= 80 / x[3].abs().max()
    x[4] = 1.25
    x = x.to(dtype)
    add = torch.randn(5, V, generator=g) if with_add else None
    x64 = _np64(x)
    a64 = None if add is None else _np64(add)
    ref = log_softmax_ref(x64, a64, MU)
    m32 = log_softmax_ref(x64, a64, MU, dtype=np.float32)
    xd = _strided(x, dev)
    ad = _strided(add, dev, pad=7) if with_add else None
    assert xd.stride(0) == V + 5 and (ad is None or ad.stride(0) == V + 7)
    out = ops.log_softmax(xd, add=ad, mu=MU)
    assert out.shape == (5, V) and out.dtype == torch.float32
    e32 = _e32(m32, ref)
    err, share = _share(out.cpu().numpy(), ref, np.maximum(4 * e32, _lsm_bound(x64, 256, out=ref)))
    print(f"[measured] log_softmax V={V} {_DT_IDS[_DT.index(dtype)]} add={with_add}: err {err:.2e} (f32 model {e32.max():.2e}) "
          f"{share:.2f} of bound")
    assert share <= 1.0, (err, e32.max(), share)


# ---- topk ------------------------------------------------------------------------------------------------------------------------
_TOPK = [(V, k) for V in (64, 257, 1000, 15360, 15361, 38400) for k in (1, 15, 63, 64)] + [(64, 64)]
_TOPK = sorted(set(_TOPK))


@pytest.mark.parametrize("V,k", _TOPK)
def test_topk_exact(dev, V, k):
    """rows drawn from a grid of 31 values -- every row full of ties, the k-th boundary cutting through one -- as a strided view;
    values bit for bit, indices in the reference order, aux gathered.  V * 4 bytes of LDS: 15360 | 15361 straddle the 60 KiB attribute
    switch, 38400 is the 150 KiB limit"""
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(V + k)
    M = 3
    x = (torch.randint(0, 31, (M, V), generator=g).float() - 15) / 2
    x[1] = 3.5          # one value throughout: indices 0 .. k - 1
    aux = torch.randn(M, V, generator=g)
    xd, auxd = _strided(x, dev), _strided(aux, dev, pad=9)
    vals, idx, aux_out = ops.topk(xd, k, aux=auxd)
    want = topk_ref(x.double().numpy(), k)
    assert np.array_equal(idx.cpu().numpy(), want), (V, k)
    assert torch.equal(vals.cpu(), torch.gather(x, 1, torch.from_numpy(want)))
    assert torch.equal(aux_out.cpu(), torch.gather(aux, 1, torch.from_numpy(want)))
    vals2, idx2, none = ops.topk(xd, k)
    assert none is None and torch.equal(vals2, vals) and torch.equal(idx2, idx)


# ---- beam_scores_topk ------------------------------------------------------------------------------------------------------------
_BS_V = [2, 40, 64, 65, 1023, 1024, 1025, 4096, 4097, 16384, 16385, 18000, 20000, 37000]
_BS = [(V, 15) for V in _BS_V if V >= 15] + [(V, k) for V in (40, 1025, 16385) for k in (1, 2, 32, 33, 64) if k <= V] \
    + [(40, 40), (2, 1), (2, 2)]


def _beam_call(dev, dec, lm, k):
    """dec [M,V] (f32 / bf16), lm f32 [M,V] | None, both as strided views -> (vals, idx, lm_at) numpy"""
    from emoasr_amd import lib, ops
    M, V = dec.shape
    dd = _strided(dec, dev)
    ld = _strided(lm, dev, pad=3) if lm is not None else None
    vals = torch.full((M, k), NAN, device=dev)
    idx = torch.full((M, k), -1, device=dev, dtype=torch.int32)
    at = torch.full((M, k), NAN, device=dev)
    lib.call("emoasr_beam_scores_topk", ops.dt(dd), M, V, k, dd.data_ptr(), dd.stride(0), None if ld is None else ld.data_ptr(),
             0 if ld is None else ld.stride(0), MU, vals.data_ptr(), idx.data_ptr(), at.data_ptr(), ops._stream())
    return vals.cpu().numpy(), idx.cpu().numpy().astype(np.int64), at.cpu().numpy()


@pytest.mark.parametrize("V,k", _BS)
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_beam_scores_topk_selection_is_exact(dev, dtype, V, k):
    """no LM; decoder entries on the grid of multiples of 1/8 in [-15, 15] (exact in bf16 and f32).  Subtracting one f32 constant from
    a row is monotone and cannot merge grid neighbours (spacing 0.125 against an ulp <= 2^-18 below 64), so the indices must be
    topk_ref's exactly: about 241 distinct values per row put ties inside a lane (v, v + 1024), across lanes and waves, and through
    the k-th boundary.  Row 1 is one value throughout: indices 0 .. k - 1."""
    g = torch.Generator().manual_seed(3 * V + k)
    M = 4
    dec = (torch.randint(-120, 121, (M, V), generator=g).float() / 8)
    dec[1] = -2.5
    dec = dec.to(dtype)
    assert torch.equal(dec.float() * 8, (dec.float() * 8).round())
    vals, idx, at = _beam_call(dev, dec, None, k)
    d64 = _np64(dec)
    want = topk_ref(d64, k)
    assert np.array_equal(idx, want), (V, k, np.argwhere(idx != want)[:4])
    assert (idx[1] == np.arange(k)).all()
    ref = log_softmax_ref(d64)
    e32 = _e32(log_softmax_ref(d64, dtype=np.float32), ref)
    bound = np.maximum(4 * e32, _lsm_bound(d64, 1024))
    err, share = _share(vals, np.take_along_axis(ref, want, 1), np.take_along_axis(bound, want, 1))
    print(f"[measured] beam_scores_topk grid V={V} k={k} {_DT_IDS[_DT.index(dtype)]}: vals err {err:.2e} (f32 model {e32.max():.2e}) "
          f"{share:.2f} of bound")
    assert share <= 1.0, (err, e32.max(), share)
    assert (at == 0).all()          # lm_at without an LM


_DUP_BASE, _DUP_OFFS = (1, 9, 30), (0, 64, 1024, 4096)


def _value_rows(V, k, dtype, g):
    """five rows: Gaussian * 3 (LM rows * 2).  Columns v, v + 64, v + 1024, v + 4096 (those below V) of three groups carry one decoder
    and one LM entry each, the decoder entry among the row's best; row 3 has -inf decoder entries, at least k finite ones left"""
    M = 5
    dec = (torch.randn(M, V, generator=g) * 3).to(dtype)
    lm = torch.randn(M, V, generator=g) * 2
    groups = []
    for gi, v in enumerate(_DUP_BASE):
        cols = [v + o for o in _DUP_OFFS if v + o < V]
        if len(cols) < 2:
            continue
        groups.append(cols)
        for m in range(M):
            top = torch.sort(dec[m].float(), descending=True).values
            dec[m, cols] = top[min(2 * gi + 1, V - 1)].to(dtype)
            lm[m, cols] = lm[m, v].clone()
    free = torch.tensor([v for v in range(V) if not any(v in cols for cols in groups)], dtype=torch.long)      # (the groups stay whole)
    n_inf = min(V - k, V // 3, len(free))
    dead = free[torch.randperm(len(free), generator=g)[:n_inf]]
    dec[3, dead] = -math.inf
    return dec, lm, groups, set(dead.tolist())


@pytest.mark.parametrize("V,k", _BS)
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_beam_scores_topk_values(dev, dtype, V, k):
    """with and without the LM row (18000: candidates walked in LDS with the LM row in LDS; 20000 and up: the LM row read from global
    memory; 37000: the largest LDS plan)"""
    g = torch.Generator().manual_seed(5 * V + k)
    dec, lm, groups, dead = _value_rows(V, k, dtype, g)
    d64, l64 = _np64(dec), _np64(lm)
    name = _DT_IDS[_DT.index(dtype)]
    for use_lm in (False, True):
        vals, idx, at = _beam_call(dev, dec, lm if use_lm else None, k)
        s64, llm64 = beam_scores_ref(d64, l64 if use_lm else None, MU)
        s32, llm32 = beam_scores_ref(d64, l64 if use_lm else None, MU, dtype=np.float32)
        e32 = _e32(s32, s64)
        bound = _lsm_bound(d64, 1024)
        if use_lm:
            b_lm = _lsm_bound(l64, 1024)
            bound = bound + MU * b_lm
        bound = np.maximum(4 * e32, bound)
        # the order statistics need the sup norm: the row's LARGEST bound (that of its most negative entry, two to three times the bound
        # at the returned entries) -- the rigorous form of the Lipschitz argument, not the value bound, which is the per-entry check
        # of vals against the float64 score at idx below
        row_bound = np.where(np.isfinite(s64), bound, 0).max(1, keepdims=True)
        assert ((idx >= 0) & (idx < V)).all()
        for m in range(idx.shape[0]):
            assert len(set(idx[m].tolist())) == k, (m, idx[m])
        assert not (set(idx[3].tolist()) & dead), "an index of a -inf entry"
        kth = -np.sort(-s64, axis=1)[:, :k]
        err1, sh1 = _share(vals, kth, row_bound)
        err2, sh2 = _share(vals, np.take_along_axis(s64, idx, 1), np.take_along_axis(bound, idx, 1))
        line = f"vals err {err1:.2e} {sh1:.2f} of bound, at idx err {err2:.2e} {sh2:.2f} of bound"
        sh3 = 0.0
        if use_lm:
            b_at = np.maximum(4 * _e32(llm32, llm64), b_lm)
            err3, sh3 = _share(at, np.take_along_axis(llm64, idx, 1), np.take_along_axis(b_at, idx, 1))
            line += f", lm_at err {err3:.2e} {sh3:.2f} of bound"
        else:
            assert (at == 0).all()
        print(f"[measured] beam_scores_topk V={V} k={k} {name} lm={use_lm}: {line} (f32 model {e32.max():.2e})")
        assert max(sh1, sh2, sh3) <= 1.0, (use_lm, sh1, sh2, sh3)
        # equal columns: a returned member brings every lower-index member with it, earlier in the row
        hits = 0
        for m in range(idx.shape[0]):
            where = {int(v): j for j, v in enumerate(idx[m])}
            for cols in groups:
                got = [where.get(c) for c in cols]
                for i, p in enumerate(got):
                    if p is not None:
                        hits += 1
                        assert all(q is not None and q < p for q in got[:i]), (m, cols, got)
        assert hits > 0 or k < 15 or not groups, "no member of an equal group among the returned"


# ---- the CTC prefix scorer, dense ------------------------------------------------------------------------------------------------
# (T, V, nb).  The recursion runs over frames start .. T - 1 in chunks of 64, start = max(out_len, 1) = 1, 1, 2, 3, 4, 5 along a chain.
# T = 1, 2: start == T inside the chain; 5: the chain's last step has out_len == T; 64: one partial chunk of 63 .. 59 frames; 65, 66:
# exactly one whole chunk (start = 1 | 2), a whole chunk and one or two frames of a second; 129, 130: two whole chunks and the start of
# a third; 200: the longest run of dependent steps.  V = 5003: another index stride.
PREFIX_CASES = [(T, 40, nb) for T in (1, 2, 5, 64, 65, 66, 129, 130, 200) for nb in (1, 3)] + [(66, 5003, 3)]


def _prefix_row_check(x, st, m, r_prev, psi, states, sc64, sc32):
    """row m of one scorer call on the device -- psi [5], states [5,T,2], computed from the float32 state r_prev -- against the float64
    scorer on the same r_prev.  Asserts the exact part and the bounded part; -> (worst share of the bound, largest error / (n u R),
    largest share of 4 n u R alone among the state rows behind 64 and more steps)"""
    T = len(x)
    start = max(st.out_len, 1)
    ref_psi, ref_st = sc64(st.hyps[m], st.cands[m], r_prev.astype(np.float64))
    o_psi, o_st = sc32(st.hyps[m], st.cands[m], r_prev)
    b_psi, b_st = prefix_bound(ref_psi, ref_st, r_prev, st.out_len, st.cands[m], EOS, BLANK)
    # exact: rows below start, blank, psi without a recursion step; r[0, 0] = x[0, c] for the empty prefix
    want_low = np.full((5, start, 2), np.float32(LOG_0))
    if st.out_len == 0:
        want_low[:, 0, 0] = x[0, st.cands[m]]
    assert np.array_equal(states[:, :start], want_low), (st.out_len, m)
    assert np.array_equal(psi[b_psi == 0], ref_psi[b_psi == 0].astype(np.float32)), (st.out_len, m)
    # exact: the fresh token stands twice in the row -- two waves, one result
    c = list(st.cands[m])
    twin = [j for j in range(5) if c.count(c[j]) == 2 and c[j] not in (EOS, BLANK, st.last[m])]
    assert len(twin) == 2 and psi[twin[0]] == psi[twin[1]] and np.array_equal(states[twin[0]], states[twin[1]])
    # bounded: max(4 e32, bound), with an e32 of their own for the log-probabilities and for LOG_0 and what was added to it
    far = np.broadcast_to(np.arange(T)[None, :, None] - start + 1 >= 64, ref_st.shape)
    worst = per_step = deep = 0.0
    for got, ref, o32, bound, far in ((psi, ref_psi, o_psi, b_psi, np.zeros(5, bool)), (states, ref_st, o_st, b_st, far)):
        err = np.abs(got.astype(np.float64) - ref)
        for live in (True, False):
            sel = ((np.abs(ref) < LIVE) == live) & (bound > 0)
            if not sel.any():
                continue
            assert np.isfinite(got[sel]).all()
            e32 = float(np.abs(o32.astype(np.float64) - ref)[sel].max())
            share = float((err[sel] / np.maximum(4 * e32, bound[sel])).max())
            assert share <= 1.0, (st.out_len, m, live, float(err[sel].max()), e32, share)
            worst = max(worst, share)
            if live:      # (bound = PREFIX_ROUNDINGS n u R)
                per_step = max(per_step, float((err[sel] * PREFIX_ROUNDINGS / bound[sel]).max()))
                if (sel & far).any():
                    deep = max(deep, float((err[sel & far] / bound[sel & far]).max()))
    return worst, per_step, deep


@pytest.mark.parametrize("T,V,nb", PREFIX_CASES)
def test_ctc_prefix_scorer_against_f64(dev, T, V, nb):
    """the initial state, then the chain of prefix_chain(T, V, nb): every step is fed the device state of the step before"""
    from emoasr_amd import ops
    from oracle.decoder import CTCPrefixScorer
    x = prefix_emissions(T, V, seed=T + V)
    sc64, sc32 = CTCPrefixScorer64(x, BLANK, EOS), CTCPrefixScorer(x, BLANK, EOS)
    xd = torch.from_numpy(x).to(dev)
    # the initial state: a running float32 sum -- row t is t additions, each rounded at no more than the magnitude of the result
    r0d = ops.ctc_prefix_init(xd, BLANK)
    r0 = r0d.cpu().numpy()
    ref0 = sc64.initial_state()
    e32_init = float(np.abs(sc32.initial_state()[:, 1].astype(np.float64) - ref0[:, 1]).max())
    assert (r0[:, 0] == np.float32(LOG_0)).all() and r0[0, 1] == x[0, BLANK]
    _, share_init = _share(r0[:, 1], ref0[:, 1], np.maximum(4 * e32_init, np.arange(T) * U24 * np.abs(ref0[:, 1])))
    assert share_init <= 1.0, share_init
    shares, prev_d, prev = [], None, None
    for st in prefix_chain(T, V, nb):
        args = (xd, _i32(st.cands, dev), _i32(st.last, dev), _i32([st.out_len] * nb, dev), BLANK, EOS)
        if prev_d is None:
            psi_d, st_d = ops.ctc_prefix_score(*args, init_state=r0d)
        else:
            psi_d, st_d = ops.ctc_prefix_score(*args, prev_states=prev_d, parent=_i32(st.parent, dev), pcand=_i32(st.pcand, dev))
        psi, states = psi_d.cpu().numpy(), st_d.cpu().numpy()
        assert psi.shape == (nb, 5) and states.shape == (nb, 5, T, 2)
        for m in range(nb):
            r_prev = r0 if prev is None else prev[st.parent[m], st.pcand[m]]
            shares.append(_prefix_row_check(x, st, m, r_prev, psi[m], states[m], sc64, sc32))
        prev_d, prev = st_d, states
    worst, per_step, deep = (max(v) for v in zip(*shares))
    print(f"[measured] ctc_prefix T={T} V={V} nb={nb}: worst share of the bound {worst:.3f} (init {share_init:.3f}); largest error / "
          f"(n u R) {per_step:.3f}, state rows behind 64 and more steps {deep:.3f} of 4 n u R")


# ---- the ragged twin -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tmax", [130, 192])
def test_ragged_ctc_prefix_scorer_past_one_chunk(dev, Tmax):
    """five searches of 1, 64, 65, 130 and 7 frames in slots of Tmax rows, two steps: equal to the dense kernel on each search's own
    frames; the slots are handed over full of NaN: rows t < T_s come back finite, rows t >= T_s are still NaN"""
    from emoasr_amd import ops
    rs = np.random.RandomState(Tmax)
    V, W, cw = 40, 2, 3
    Ts = [1, 64, 65, 130, 7]
    S = len(Ts)
    offs = [0] + list(np.cumsum(Ts))
    x = torch.from_numpy(np.log(rs.dirichlet(np.ones(V) * 0.5, size=offs[-1])).astype(np.float32)).to(dev)
    xoff = _i32(offs, dev)
    nb = S * W
    real = [v for v in range(V) if v not in (BLANK, EOS)]
    prev = torch.full((nb, cw, Tmax, 2), NAN, device=dev)
    ops.ctc_prefix_init_ragged(x, xoff, BLANK, prev, W * cw * Tmax * 2)
    c0 = rs.choice(real, (nb, cw))
    c0[:, 1] = EOS
    c0[0, 2] = BLANK
    c0[3, 2] = BLANK
    c0d = _i32(c0, dev)
    last0, olen0 = _i32([EOS] * nb, dev), _i32([0] * nb, dev)
    par0, pc0 = _i32([s * W for s in range(S) for _ in range(W)], dev), _i32([0] * nb, dev)
    st0 = torch.full((nb, cw, Tmax, 2), NAN, device=dev)
    psi0, st0 = ops.ctc_prefix_score_ragged(x, xoff, W, Tmax, c0d, last0, olen0, BLANK, EOS, prev, par0, pc0, states=st0)
    # step 1: parents mixed inside every search (one used twice in some), the parent's candidate 0 or 2; one candidate repeats the
    # last token
    lpar = rs.randint(0, W, nb)
    pc1 = np.where(rs.randint(0, 2, nb) == 1, 2, 0)
    gpar = np.array([(m // W) * W + lpar[m] for m in range(nb)])
    last1 = c0[gpar, pc1]
    c1 = rs.choice(real, (nb, cw))
    c1[:, 0] = last1
    c1[:, 2] = EOS
    c1d, last1d, olen1 = _i32(c1, dev), _i32(last1, dev), _i32([1] * nb, dev)
    st1 = torch.full((nb, cw, Tmax, 2), NAN, device=dev)
    psi1, st1 = ops.ctc_prefix_score_ragged(x, xoff, W, Tmax, c1d, last1d, olen1, BLANK, EOS, st0, _i32(gpar, dev), _i32(pc1, dev),
                                            states=st1)
    for s in range(S):
        rows, T = slice(s * W, s * W + W), Ts[s]
        xs = x[offs[s]:offs[s + 1]].contiguous()
        r0 = ops.ctc_prefix_init(xs, BLANK)
        assert torch.equal(prev[s * W, 0, :T], r0), s
        assert bool(torch.isnan(prev[s * W, 0, T:]).all()) and bool(torch.isnan(prev[s * W, 1:]).all()), s
        p0, s0 = ops.ctc_prefix_score(xs, c0d[rows].contiguous(), last0[rows], olen0[rows], BLANK, EOS, init_state=r0)
        assert torch.equal(psi0[rows], p0) and torch.equal(st0[rows, :, :T], s0), s
        p1, s1 = ops.ctc_prefix_score(xs, c1d[rows].contiguous(), last1d[rows], olen1[rows], BLANK, EOS, prev_states=s0,
                                      parent=_i32(lpar[s * W:(s + 1) * W], dev), pcand=_i32(pc1[s * W:(s + 1) * W], dev))
        assert torch.equal(psi1[rows], p1) and torch.equal(st1[rows, :, :T], s1), s
        for st in (st0, st1):
            assert bool(torch.isfinite(st[rows, :, :T]).all()) and bool(torch.isnan(st[rows, :, T:]).all()), s
    assert bool(torch.isfinite(psi0).all()) and bool(torch.isfinite(psi1).all())


# ---- emoasr_beam_cache_gather ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 1, 7, 12])
@pytest.mark.parametrize("d", [8, 256])
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_beam_cache_gather_exact(dev, dtype, d, pos):
    """rows of 16, 32, 512 and 1024 bytes; parents a permutation, one parent for all, the identity.  dst[l, b, t] = src[l, parent[b], t]
    for t < pos; rows t >= pos and the words behind the caches keep their sentinel; src is unchanged; K and V cache"""
    from emoasr_amd import lib, ops
    nl, nb, Lmax = 2, 5, 12
    g = torch.Generator().manual_seed(d + pos)
    n = nl * nb * Lmax * d
    src = [torch.randn(nl, nb, Lmax, d, generator=g).to(dtype).to(dev) for _ in range(2)]
    keep = [t.clone() for t in src]
    posd = _i32([pos], dev)
    for parent in ([3, 0, 4, 1, 2], [2, 2, 2, 2, 2], [0, 1, 2, 3, 4]):
        flat = [torch.full((n + 64,), -7.0, dtype=dtype, device=dev) for _ in range(2)]
        dst = [f[:n].view(nl, nb, Lmax, d) for f in flat]
        pard = _i32(parent, dev)
        lib.call("emoasr_beam_cache_gather", ops.dt(src[0]), nl, nb, Lmax, d, src[0].data_ptr(), src[1].data_ptr(), dst[0].data_ptr(),
                 dst[1].data_ptr(), pard.data_ptr(), posd.data_ptr(), ops._stream())
        for i in range(2):
            assert torch.equal(dst[i][:, :, :pos], src[i][:, parent][:, :, :pos]), (i, parent)
            assert bool((dst[i][:, :, pos:] == -7.0).all()) and bool((flat[i][n:] == -7.0).all()), (i, parent)
            assert torch.equal(src[i], keep[i])


# ---- attn_step -------------------------------------------------------------------------------------------------------------------
_ATTN = [(d, H, Lmax, pos) for d, H in ((256, 4), (256, 2), (64, 8), (128, 4)) for Lmax in (64, 200)
         for pos in sorted({0, 63, 64, 65, 127, 128, Lmax - 1}) if pos < Lmax]


@pytest.mark.parametrize("d,H,Lmax,pos", _ATTN)
def test_attn_step_against_f64(dev, d, H, Lmax, pos):
    """dk = 64, 128, 8, 32 (as many, more and fewer columns than lanes); pos on both sides of the 64-position trips.  The caches get
    the new k / v at row pos, bit for bit, and nothing else; the output is within one bf16 ulp + 4 e32 of the float64 attention over
    the bf16 inputs"""
    from emoasr_amd import ops
    bf = torch.bfloat16
    nb = 3
    g = torch.Generator().manual_seed(d + 7 * H + Lmax + pos)
    qkv = torch.randn(nb, 3 * d, generator=g).to(bf)
    kc, vc = torch.randn(nb, Lmax, d, generator=g).to(bf), torch.randn(nb, Lmax, d, generator=g).to(bf)
    ref, k_ref, v_ref = attn_step_ref(_np64(qkv), _np64(kc), _np64(vc), pos, H)
    m32, _, _ = attn_step_ref(_np64(qkv), _np64(kc), _np64(vc), pos, H, dtype=np.float32)
    kd, vd = kc.to(dev), vc.to(dev)
    out = ops.attn_step(qkv.to(dev), kd, vd, _i32([pos], dev), H)
    assert out.dtype == bf and out.shape == (nb, d)
    assert np.array_equal(_np64(kd), k_ref) and np.array_equal(_np64(vd), v_ref)      # row pos = the new k / v, the rest untouched
    e32 = float(_e32(m32, ref).max())
    err, share = _share(_np64(out), ref, P8 * np.abs(ref) + 4 * e32)
    print(f"[measured] attn_step d={d} H={H} Lmax={Lmax} pos={pos}: err {err:.2e} (f32 model {e32:.2e}) {share:.2f} of bound")
    assert share <= 1.0, (err, e32, share)
