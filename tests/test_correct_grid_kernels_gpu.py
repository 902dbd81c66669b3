"""The correction grid's kernels (csrc/correct.hip) against numpy (tests/correct_grid_ref.py) and against the single-weight kernel.

  correct_mask_grid   exact: masked inputs, counts and both row lists in (threshold, utterance, token) order.  Token counts cross
                      the 64- and 128-token passes of the wave; one batch holds ntok == 0 and ntok == T; thresholds below and above
                      every confidence and one EQUAL to a confidence (not masked: the comparison is strict).
  correct_fuse_grid   ids and values of every weight BITWISE equal to ops.correct_fuse with that weight (same arithmetic, same
                      reduction order); against fuse_ref in float64 the existing kernel's bars: ids where the top-2 margin exceeds
                      1e-6, values to rtol 2e-6."""
import numpy as np
import pytest
import torch

from tests.correct_grid_ref import fuse_grid_ref, mask_grid_ref
from tests.test_correct_gpu import _dev_rows

pytestmark = pytest.mark.gpu

MASK, PAD = 39, 0


# ---- correct_mask_grid ---------------------------------------------------------------------------------------------------------------
def _mask_case(T, NT):
    rng = np.random.default_rng(10 * T + NT)
    B = 3
    ntok = [T, 0, max(T - 3, 1)]
    hyp = rng.integers(1, 39, (B, T))
    conf = rng.uniform(0.05, 0.95, (B, T)).astype(np.float32)
    frame = np.sort(rng.integers(0, T, (B, T)), axis=1)
    conf[1] = np.nan                                     # (ntok == 0: never read; a NaN compares false anyway)
    hyp[2, ntok[2]:], conf[2, ntok[2]:] = 10 ** 6, 0.0   # past the count: garbage that would be masked if it were read
    equal = float(conf[0, T // 2])                       # a threshold EQUAL to a confidence: that token is not masked
    ths = [equal] if NT == 1 else [0.01, 0.3, equal, 0.7, 0.99]
    return hyp, ntok, conf, frame, ths


@pytest.mark.parametrize("NT", [1, 5])
@pytest.mark.parametrize("T", [5, 70, 130])
def test_correct_mask_grid(dev, T, NT):
    from emoasr_amd import ops
    hyp, ntok, conf, frame, ths = _mask_case(T, NT)
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32, device=dev)
    ys, num, lm_rows, asr_rows = ops.correct_mask_grid(i32(hyp), i32(ntok), torch.from_numpy(conf).to(dev), i32(frame),
                                                       torch.tensor(ths, dtype=torch.float32, device=dev), MASK, PAD)
    w_ys, w_num, w_lm, w_asr = mask_grid_ref(hyp, ntok, conf, frame, ths, MASK, PAD)
    assert ys.shape == (NT, 3, T) and ys.dtype == torch.int32 and num.shape == (NT, 3)
    assert (ys.cpu().numpy() == w_ys).all()
    assert (num.cpu().numpy() == w_num).all()
    n = int(w_num.sum())
    assert lm_rows.numel() == asr_rows.numel() == NT * 3 * T
    assert lm_rows[:n].cpu().tolist() == w_lm.tolist() and asr_rows[:n].cpu().tolist() == w_asr.tolist()
    k = ths.index(float(conf[0, T // 2]))
    assert w_ys[k, 0, T // 2] == hyp[0, T // 2]          # the equal threshold
    assert (w_num[:, 1] == 0).all() and (w_ys[:, 1] == PAD).all()
    if NT == 5:
        assert w_num[0].sum() == 0 and w_num[4].tolist() == [T, 0, max(T - 3, 1)]      # masks nothing / everything


# ---- glu_fwd_masked (engine.mask_padding: what lets a padded batch through correct_batch equal the utterances alone) ------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_glu_fwd_masked_is_glu_fwd_with_zeros_past_the_lengths(dev, dtype):
    from emoasr_amd import ops
    B, T, C = 3, 37, 24
    g = torch.randn(B * T, 2 * C, generator=torch.Generator().manual_seed(1)).to(dev, dtype)
    lens = [T, 0, 11]
    got = ops.glu_fwd_masked(g, B, T, torch.tensor(lens, dtype=torch.int32, device=dev)).view(B, T, C)
    want = ops.glu_fwd(g).view(B, T, C).clone()
    for b, n in enumerate(lens):
        want[b, n:] = 0
    assert torch.equal(got, want)


# ---- correct_fuse_grid ---------------------------------------------------------------------------------------------------------------
WEIGHTS = {1: [0.3], 3: [0.0, 0.5, 1.0],
           16: [0.0, 1.0] + [float(w) for w in np.random.default_rng(16).uniform(0, 1, 14).astype(np.float32)]}
DTS = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)]


def _fuse_case(n, V, dt_a, dt_l):
    """asr [R, V], lm [n, V + 1] rounded to their dtypes (as float64), recogniser rows with repeats, n_cols = V - 3"""
    rng = np.random.default_rng(100 * n + V)
    R = n + 2
    asr = rng.standard_normal((R, V)) * 2.0
    lm = rng.standard_normal((n, V + 1)) * 2.0
    for x in (asr, lm):      # the leading column of every row leads by 0.5 at least (bf16 rounding cannot make the top two equal)
        x[np.arange(len(x)), x.argmax(axis=1)] += rng.uniform(0.5, 1.5, len(x))
    asr[:, rng.integers(0, V)] = -np.inf
    lm[:, rng.integers(0, V + 1)] = -np.inf
    rows = rng.integers(0, R, n)
    rows[-1] = rows[0]                                   # a recogniser row read by two LM rows
    asr = torch.from_numpy(asr).to(dt_a).double().numpy()
    lm = torch.from_numpy(lm).to(dt_l).double().numpy()
    return asr, lm, rows, V - 3


@pytest.mark.parametrize("V", [40, 257, 2056])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("dts", DTS, ids=["f32", "f32+bf16", "bf16"])
def test_correct_fuse_grid(dev, dts, n, V):
    from emoasr_amd import ops
    asr, lm, rows, n_cols = _fuse_case(n, V, *dts)
    lse = torch.logsumexp(torch.from_numpy(asr), dim=-1).float().to(dev)
    rows_d = torch.from_numpy(rows).to(torch.int32).to(dev)
    worst = 0.0
    # contiguous rows, rows with an odd leading dimension (unaligned), rows padded to a multiple of 8 elements (the 16-byte loads)
    for ld_a, ld_l in ((None, None), (V + 3 + V % 2, V + 4 + V % 2), ((V + 7) // 8 * 8 + 8, (V + 8) // 8 * 8)):
        a_d, l_d = _dev_rows(asr, dts[0], dev, ld_a), _dev_rows(lm, dts[1], dev, ld_l)
        for NW, ws in WEIGHTS.items():
            ids, val = ops.correct_fuse_grid(a_d, lse, l_d, ws, n_cols, asr_rows=rows_d)
            assert ids.shape == (NW, n) and ids.dtype == torch.int32 and val.dtype == torch.float32
            for m, w in enumerate(ws):
                i1, v1 = ops.correct_fuse(a_d, lse, l_d, w, n_cols, asr_rows=rows_d)
                assert torch.equal(ids[m], i1), (NW, w, ids[m], i1)
                assert torch.equal(val[m].view(torch.int32), v1.view(torch.int32)), (NW, w, val[m], v1)      # bit for bit
            w_ids, w_val, margin = fuse_grid_ref(asr[rows], lm, ws, n_cols)
            ok = margin > 1e-6
            assert (ids.cpu().numpy()[ok] == w_ids[ok]).all()
            np.testing.assert_allclose(val.cpu().numpy(), w_val, rtol=2e-6)
            worst = max(worst, float((np.abs(val.cpu().numpy() - w_val) / w_val).max()))
    print(f"[measured] correct_fuse_grid n={n} V={V} {dts}: value rel err {worst:.2e} (bar 2e-06)")


@pytest.mark.parametrize("V", [5, 40, 1003])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_correct_fuse_grid_ties_go_to_the_lowest_column(dev, dtype, V):
    """the tie case of test_correct_fuse_ties_go_to_the_lowest_column, all three weights in one launch"""
    from emoasr_amd import ops
    rng = np.random.default_rng(V)
    n = 6
    asr = torch.from_numpy(rng.standard_normal((n, V))).to(dtype)
    lm = torch.from_numpy(rng.standard_normal((n, V + 1))).to(dtype)
    lo = [0, 1, V // 2 - 1, V - 2, 0, 2]
    hi = [V - 1, 2, V // 2 + 1, V - 1, 1, V - 1]
    for i in range(n):                     # two columns equal in both inputs and above the rest: equal mixed values, bit for bit
        asr[i, lo[i]] = asr[i, hi[i]] = 6.0
        lm[i, lo[i]] = lm[i, hi[i]] = 5.0
    lse = torch.logsumexp(asr.double(), dim=-1).float()
    ids, _ = ops.correct_fuse_grid(asr.to(dev), lse.to(dev), lm.to(dev), [0.0, 0.3, 1.0], V)
    assert ids.cpu().tolist() == [lo, lo, lo]
    lm[:, V] = 30.0                        # a column only the LM likes, outside n_cols, is not a candidate
    ids, _ = ops.correct_fuse_grid(asr.to(dev), lse.to(dev), lm.to(dev), [1.0, 0.5], V)
    assert ids.cpu().tolist() == [lo, lo]


def test_correct_fuse_grid_chunks_above_sixteen_weights(dev):
    from emoasr_amd import ops
    asr, lm, rows, n_cols = _fuse_case(5, 257, torch.float32, torch.float32)
    lse = torch.logsumexp(torch.from_numpy(asr), dim=-1).float().to(dev)
    a_d, l_d = _dev_rows(asr, torch.float32, dev), _dev_rows(lm, torch.float32, dev)
    rows_d = torch.from_numpy(rows).to(torch.int32).to(dev)
    ws = [k / 16 for k in range(17)]
    assert len(ws) > ops.CORRECT_MAX_WEIGHTS
    ids, val = ops.correct_fuse_grid(a_d, lse, l_d, ws, n_cols, asr_rows=rows_d)
    assert ids.shape == (17, 5)
    for m, w in enumerate(ws):
        i1, v1 = ops.correct_fuse(a_d, lse, l_d, w, n_cols, asr_rows=rows_d)
        assert torch.equal(ids[m], i1) and torch.equal(val[m].view(torch.int32), v1.view(torch.int32)), (m, w)
    with pytest.raises(Exception):         # the entry point itself takes 16 at the most
        from emoasr_amd import lib
        from emoasr_amd.ops import _DT, _p, _stream
        w17 = torch.tensor(ws, dtype=torch.float32)
        o_i, o_v = torch.empty(17, 5, device=dev, dtype=torch.int32), torch.empty(17, 5, device=dev)
        lib.call("emoasr_correct_fuse_grid", _DT[a_d.dtype], _DT[l_d.dtype], 5, 257, 258, n_cols, _p(a_d), a_d.stride(0), _p(lse),
                 _p(rows_d), 7, _p(l_d), l_d.stride(0), _p(w17), 17, _p(o_i), _p(o_v), _stream())
