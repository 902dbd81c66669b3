"""tests/conv_ref.py on the CPU: the float64 reference equals torch.autograd, the closed forms hold for it, the float32 model is
inside the bounds on every case of every table, and every mutant leaves them on a named case."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R
from tests.norm_ref import BF, F32, F64, colsum_bound, elem_bound, share

DTYPES = [F32, BF]
NOMINAL_CUS = 256      # the RULE shapes follow the device's CU count on the GPU; here the MI355X's


def _autograd(x, w, bias, dy):
    B, T, C = x.shape
    K = w.shape[1]
    x, w, bias = x.clone().requires_grad_(), w.clone().requires_grad_(), bias.clone().requires_grad_()
    y = F.conv1d(x.transpose(1, 2), w[:, None, :], bias, padding=(K - 1) // 2, groups=C).transpose(1, 2)
    y.backward(dy)
    return y.detach(), x.grad, w.grad, bias.grad


@pytest.mark.parametrize("shape", [(2, 70, 24, 1), (2, 7, 12, 31), (3, 33, 20, 15)], ids=str)      # K = 1; T < pad; several tiles' worth
def test_reference_equals_autograd(shape):
    B, T, C, K = shape
    inp = R.conv_inputs(("auto", B, T, C, K, "randn"), F32)
    x, dy, w, bias = inp.x.double(), inp.dy.double(), inp.w.double(), inp.bias.double()
    y, dx, dw, db = _autograd(x, w, bias, dy)
    assert (R.dwconv_fwd(x, w, bias) - y).abs().max() < 1e-11
    assert (R.dwconv_fwd(x, w, None) - (y - bias)).abs().max() < 1e-11
    assert (R.dwconv_bwd_x(dy, w) - dx).abs().max() < 1e-11
    rdw, rdb, adw, adb = R.dwconv_bwd_w(dy, x, K)
    assert (rdw - dw).abs().max() < 1e-11 and (rdb - db).abs().max() < 1e-11
    assert bool((adw >= rdw.abs() - 1e-11).all()) and (adb - dy.abs().sum((0, 1))).abs().max() < 1e-11
    # GLU
    g = inp.g.double().reshape(B * T, 2 * C).clone().requires_grad_()
    d = inp.ds.double().reshape(B * T, C)
    out = F.glu(g, -1)
    out.backward(d)
    assert (R.glu_fwd(g.detach()) - out.detach()).abs().max() < 1e-11
    assert (R.glu_bwd(g.detach(), d) - g.grad).abs().max() < 1e-11
    lens = torch.tensor([0, T][:B] + [T - 1] * (B - 2))
    m = R.glu_fwd_masked(inp.g.double(), lens)
    for b in range(B):
        assert torch.equal(m[b, :lens[b]], out.detach().reshape(B, T, C)[b, :lens[b]]) and bool((m[b, lens[b]:] == 0).all())


@pytest.mark.parametrize("B,T,K", [(2, 70, 31), (2, 7, 31), (1, 1, 1), (3, 33, 7), (2, 289, 15)])
def test_closed_forms_hold_for_the_reference(B, T, K):
    C = 3
    one, w = torch.ones(B, T, C, dtype=F64), torch.ones(C, K, dtype=F64)
    y = R.dwconv_fwd(one, w, None)
    assert torch.equal(y, R.tap_counts(T, K).double()[None, :, None].expand(B, T, C))
    assert torch.equal(R.dwconv_bwd_x(one, w), y)
    dw, db, _, _ = R.dwconv_bwd_w(one, one, K)
    assert torch.equal(dw, R.dw_counts(B, T, K).double()[None, :].expand(C, K))
    assert torch.equal(db, torch.full((C,), float(B * T), dtype=F64))
    assert float(y.max()) <= 31


def _conv_model_shares(inp, mutant=None):
    """the float32 model in kernel form against the bounds of every convolution tensor"""
    res = dict(R.check_fwd(inp, R.model_fwd(inp, mutant)))
    res["y nobias"] = R.check_fwd(inp, R.model_fwd(inp, mutant, bias=False), bias=False)["y"]
    res.update(R.check_bwd_x(inp, R.model_bwd_x(inp, mutant)))
    res.update(R.check_bwd_w(inp, *R.model_bwd_w(inp, mutant)))
    dw, db = R.model_bwd_w(inp, mutant, accumulate=False)
    res.update({k + " stored": v for k, v in R.check_bwd_w(inp, dw, db, accumulate=False).items()})
    return res


ALL_CONV = R.DW_CASES + R.STRIPS + R.OPTIONS + R.REDUCE + R.rule_cases(NOMINAL_CUS)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ALL_CONV, ids=R.case_id)
def test_model_is_inside_the_bounds_conv(case, dtype):
    res = _conv_model_shares(R.conv_inputs(case, dtype))
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", R.GLU_CASES + R.GLU_MASKED_CASES, ids=R.case_id)
def test_model_is_inside_the_bounds_glu(case, dtype):
    inp = R.glu_inputs(case, dtype)
    for op in (("masked",) if case[0] == "glum" else ("fwd", "bwd")):
        got = R.model_glu(inp, op)
        assert bool(torch.isfinite(got).all())
        res = R.check_glu(inp, op, got)
        assert max(res.values()) <= 1.0, (op, res)


def test_hard_glu_values_are_what_the_table_says():
    inp = R.glu_inputs(("glu", 301, 12, "hard"), F32)
    a, b = inp.g[:, :12], inp.g[:, 12:]
    for v in R.GLU_GATES + R.GLU_GATES_F32:
        for av in (0.0, 1e4, -1e4):
            assert bool(((b == v) & (a == av)).any()), (v, av)
    assert not bool((R.glu_inputs(("glu", 301, 12, "hard"), BF).g.abs() == 104).any())


def test_rule_shapes_follow_the_cu_count():
    for cus in (64, 256, 304):
        a, b = R.rule_cases(cus)
        assert R.rule_S(*a[1:4], cus) >= 2 and R.rule_S(a[1] - 1, *a[2:4], cus) == 1
        assert R.rule_S(*b[1:4], cus) == 8 and R.rule_S(b[1] - 1, *b[2:4], cus) < 8


_K7, _K15, _LEAK = ("taps", 2, 70, 24, 7, "randn"), ("taps", 2, 70, 24, 15, "randn"), ("batch", 3, 33, 24, 31, "edges")
_GLU = ("glu", 301, 12, "randn")
# mutant -> (case, the tensors that must leave their bounds)
MUTANT_CASES = {
    "pad15": (_K7, ("y", "dx", "dw")),
    "no_flip": (_K15, ("dx",)),
    "halo_leak": (_LEAK, ("y", "dx", "dw")),
    "last_tile": (_K15, ("dw", "db")),
    "bwd_x_bias": (_K15, ("dx",)),
    "overwrite": (_K15, ("dw", "db")),
    "glu_swapped": (_GLU, ("out", "din")),
    "glu_gate_no_a": (_GLU, ("din",)),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("mutant", [m for m in R.MUTANTS if m])
def test_every_mutant_leaves_the_bounds(mutant, dtype):
    """pad15         taps-2-70-24-7-randn     y, dx, dw      (pad 3 is meant)
    no_flip          taps-2-70-24-15-randn    dx
    halo_leak        batch-3-33-24-31-edges   y, dx, dw      (the neighbour's |x| = 64 frame inside the window)
    last_tile        taps-2-70-24-15-randn    dw, db         (frames 64 .. 69)
    bwd_x_bias       taps-2-70-24-15-randn    dx
    overwrite        taps-2-70-24-15-randn    dw, db         (the start values are lost)
    glu_swapped      glu-301-12-randn         out, din
    glu_gate_no_a    glu-301-12-randn         din
    and every tensor the mutant does not touch stays inside"""
    case, tensors = MUTANT_CASES[mutant]
    assert case in R.DW_CASES + R.GLU_CASES
    if case[0] == "glu":
        inp = R.glu_inputs(case, dtype)
        res = {**R.check_glu(inp, "fwd", R.model_glu(inp, "fwd", mutant)), **R.check_glu(inp, "bwd", R.model_glu(inp, "bwd", mutant))}
        clean = {**R.check_glu(inp, "fwd", R.model_glu(inp, "fwd")), **R.check_glu(inp, "bwd", R.model_glu(inp, "bwd"))}
    else:
        inp = R.conv_inputs(case, dtype)
        res, clean = _conv_model_shares(inp, mutant), _conv_model_shares(inp)
    assert max(clean.values()) <= 1.0
    for k in tensors:
        assert res[k] > 1.0, (mutant, k, res)


def test_bounds_are_the_suites_own():
    assert R.elem_bound is elem_bound and R.colsum_bound is colsum_bound and R.share is share
