"""tests/lstm_ref.py pinned without a GPU: the float64 restatement against torch.nn.LSTM (unidirectional with and without a state,
bidirectional over pack_padded_sequence) and against autograd (gate-pre-activation gradients, the layer's weight gradients with
the h0 term of W_hh), and the bounds of tests/test_lstm_kernels_gpu.py from both sides: the float32 model with the kernels'
documented roundings stays inside them on every case of the GPU sweep, and every planted error leaves them."""
import pytest
import torch
import torch.nn as nn

from tests import lstm_ref as R
from tests.rnn_util import packed_bilstm

F64 = torch.float64


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _uni_setup(with_state, U=5, B=4, nin=6, H=8, seed=3):
    torch.manual_seed(seed)
    m = nn.LSTM(nin, H).double()
    x = torch.randn(U, B, nin, dtype=F64)
    h0, c0 = (torch.randn(B, H, dtype=F64) * 0.5, torch.randn(B, H, dtype=F64) * 0.5) if with_state else (None, None)
    return m, x, h0, c0


@pytest.mark.parametrize("with_state", [False, True], ids=["zero_state", "h0c0"])
def test_unidirectional_forward_is_torch_lstm(with_state):
    m, x, h0, c0 = _uni_setup(with_state)
    with torch.no_grad():
        y, (hn, cn) = m(x, (h0[None], c0[None]) if with_state else None)
        pre = x @ m.weight_ih_l0.t() + m.bias_ih_l0 + m.bias_hh_l0
        f = R.seq_fwd(pre, m.weight_hh_l0, h0, c0)
    assert _close(f.h, y) and _close(f.h[-1], hn[0]) and _close(f.c[-1], cn[0])
    assert torch.equal(f.hseq, f.h) and torch.equal(f.cseq, f.c) and torch.equal(f.gact, f.gates)      # no rounding asked for


@pytest.mark.parametrize("with_state", [False, True], ids=["zero_state", "h0c0"])
def test_unidirectional_backward_and_layer_gradients_are_autograd(with_state):
    m, x, h0, c0 = _uni_setup(with_state)
    U, B, _ = x.shape
    dh = torch.randn(U, B, 8, dtype=F64)
    x.requires_grad_(True)
    bias = (m.bias_ih_l0 + m.bias_hh_l0).detach().requires_grad_(True)
    pre = x @ m.weight_ih_l0.t() + bias
    pre.retain_grad()
    f = R.seq_fwd(pre, m.weight_hh_l0, h0, c0)
    (f.h * dh).sum().backward()
    with torch.no_grad():
        dgp = R.seq_bwd(dh, f.gates, f.c, c0, m.weight_hh_l0)
        assert _close(dgp, pre.grad)
        g_w_ih, g_w_hh, g_b, dx = R.layer_bwd(dgp, x, f.h, h0, m.weight_ih_l0)
        assert _close(g_w_ih, m.weight_ih_l0.grad) and _close(g_b, bias.grad) and _close(dx, x.grad)
        assert _close(g_w_hh, m.weight_hh_l0.grad)
        if with_state:   # (and the h0 term is what makes it so)
            assert not _close(R.layer_bwd(dgp, x, f.h, None, m.weight_ih_l0)[1], m.weight_hh_l0.grad, 1e-3)


def _bi_setup(lens, T, nin=5, H=6, seed=4):
    torch.manual_seed(seed)
    m = nn.LSTM(nin, H, batch_first=True, bidirectional=True).double()
    x = torch.randn(len(lens), T, nin, dtype=F64)
    pre = torch.cat((x @ m.weight_ih_l0.t() + m.bias_ih_l0 + m.bias_hh_l0,
                     x @ m.weight_ih_l0_reverse.t() + m.bias_ih_l0_reverse + m.bias_hh_l0_reverse), -1)
    return m, x, pre, (m.weight_hh_l0, m.weight_hh_l0_reverse)


@pytest.mark.parametrize("lens", [[7, 1, 6, 2, 7], [1, 7], [3, 3, 7, 5]], ids=str)
def test_bidirectional_layer_is_torch_lstm_over_a_packed_sequence(lens):
    T = 7
    m, x, pre, w = _bi_setup(lens, T)
    L = torch.tensor(lens)
    pre = pre.detach().requires_grad_(True)
    f = R.bi_fwd(pre, w, L)
    y = f.hseq[0] + f.hseq[1]
    assert _close(y.detach(), packed_bilstm(m, x, lens).detach())
    fm = R.frames(L, T)
    for t in (f.hseq, f.hprev, f.cseq, f.gact):
        assert bool((t.detach()[:, ~fm] == 0).all())
    assert torch.equal(f.hprev.detach(), R.bi_hprev_of(f.hseq.detach(), L))
    # the analytic backward is autograd's gradient w.r.t. pre; padded frames exact zeros
    dy = torch.randn(len(lens), T, 6, dtype=F64)
    (y * dy).sum().backward()
    with torch.no_grad():
        dg = R.bi_bwd(dy, f.gact, f.cseq, w, L)
    H4 = dg.shape[-1]
    assert _close(dg[0], pre.grad[..., :H4]) and _close(dg[1], pre.grad[..., H4:])
    assert bool((dg[:, ~fm] == 0).all()) and bool((pre.grad[~fm] == 0).all())
    # the W_hh gradient is ONE product dg^T . hprev per direction
    for d, wd in enumerate(w):
        assert _close(dg[d].reshape(-1, H4).t() @ f.hprev[d].reshape(-1, 6).detach(), wd.grad)


# ---- the bounds admit a correct kernel: the float32 model with the kernels' roundings, on every case of the GPU sweep ---------------
@pytest.mark.parametrize("case", R.UNI_CASES, ids=R.case_id)
def test_model_of_the_unidirectional_kernels_is_inside_the_bounds(case):
    inp = R.uni_inputs(case)
    res = R.check_uni(inp, *R.model_uni(inp))
    print(f"[model] lstm uni {R.case_id(case)}: " + ", ".join(f"{k} {v:.2f}" for k, v in res.items()))
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("case", R.BI_CASES, ids=R.case_id)
def test_model_of_the_bidirectional_kernels_is_inside_the_bounds(case):
    inp = R.bi_inputs(case)
    out = R.model_bi(inp)
    if case[0] == "hard":      # the planted units drive the cell state to |c| = len
        assert float(out[2].abs().max()) > min(case[2], 6) - 0.5
    res = R.check_bi(inp, *out)
    print(f"[model] lstm bi {R.case_id(case)}: " + ", ".join(f"{k} {v:.2f}" for k, v in res.items()))
    assert max(res.values()) <= 1.0, res


def test_forward_bounds_hold_with_pre_scaled_by_8():
    for case in (("rows", 3, 17, 64, "both"), ("hidden", 3, 33, 512, "both")):
        inp = R.uni_inputs(case)
        inp.pre = (inp.pre * 8).to(R.BF).float()
        res = R.check_uni(inp, *R.model_uni(inp))
        assert max(res.values()) <= 1.0, res


# ---- the bounds reject a wrong kernel: each mutant at the smallest case that can show it ------------------------------------------
_UNI_MUTANTS = [
    ("swap_if", None, ("state", 3, 17, 64, "none")),
    ("row_plus1", None, ("rows", 3, 17, 64, "both")),
    ("c0_ignored", None, ("state", 3, 17, 64, "c0")),
    (None, "c0_ignored", ("state", 3, 17, 64, "c0")),
    ("slice_drop", None, ("hidden", 3, 17, 32, "both")),
    ("row32", None, ("rows", 3, 33, 64, "both")),
    (None, "partial_tail", ("hidden", 3, 17, 32, "both")),
    (None, "partial_tail", ("hidden", 3, 17, 160, "both")),
]
_BI_MUTANTS = [
    ("swap_if", None, ("rows", 1, 3, 64, "mixed", 0)),
    ("row_plus1", None, ("rows", 17, 3, 64, "mixed", 0)),
    ("rev_plus1", None, ("rows", 17, 3, 64, "mixed", 0)),
    ("rev_minus1", None, ("rows", 17, 3, 64, "mixed", 0)),
    ("c_first", None, ("rows", 1, 3, 64, "mixed", 0)),
    (None, "c_first", ("rows", 17, 3, 64, "mixed", 0)),
    (None, "partial_tail", ("hidden", 17, 3, 32, "mixed", 0)),
    (None, "partial_tail", ("hidden", 17, 3, 160, "mixed", 0)),
]


@pytest.mark.parametrize("mf,mb,case", _UNI_MUTANTS, ids=lambda v: R.case_id(v) if isinstance(v, tuple) else str(v))
def test_unidirectional_mutants_leave_the_bounds(mf, mb, case):
    assert case in R.UNI_CASES
    inp = R.uni_inputs(case)
    res = R.check_uni(inp, *R.model_uni(inp, mf, mb))
    print(f"[mutant] lstm uni {mf or mb}: " + ", ".join(f"{k} {v:.2f}" for k, v in res.items()))
    hit = max(res[k] for k in (("dgp",) if mb else ("gact", "c", "h")))
    assert hit > 1.0, res
    if mb:     # a backward mutant leaves the forward alone
        assert max(res[k] for k in ("gact", "c", "h")) <= 1.0


@pytest.mark.parametrize("mf,mb,case", _BI_MUTANTS, ids=lambda v: R.case_id(v) if isinstance(v, tuple) else str(v))
def test_bidirectional_mutants_leave_the_bounds(mf, mb, case):
    assert case in R.BI_CASES
    inp = R.bi_inputs(case)
    out = R.model_bi(inp, mf, mb)
    if mf == "row_plus1":      # (this one also breaks the exact hprev check; the bounds must catch it on their own)
        out = (out[0], R.bi_hprev_of(out[0], inp.lens), *out[2:])
    res = R.check_bi(inp, *out)
    print(f"[mutant] lstm bi {mf or mb}: " + ", ".join(f"{k} {v:.2f}" for k, v in res.items()))
    hit = max(res[k] for k in (("dg",) if mb else ("gact", "c", "h")))
    assert hit > 1.0, res
    if mb:
        assert max(res[k] for k in ("gact", "c", "h")) <= 1.0


def test_a_wrong_hprev_row_fails_the_exact_check():
    inp = R.bi_inputs(("rows", 17, 3, 64, "mixed", 0))
    hseq, hprev, cseq, gact, dg = R.model_bi(inp)
    hprev = hprev.clone()
    hprev[1, 3, 0] = hprev[1, 4, 0]
    with pytest.raises(AssertionError, match="hprev"):
        R.check_bi(inp, hseq, hprev, cseq, gact, dg)
