"""tests/norm_ref.py pinned without a GPU: the float64 restatements against torch.autograd in float64 (F.layer_norm, F.batch_norm +
F.silu), and the bounds of tests/test_norm_kernels_gpu.py from both sides: the float32 model (sequential sums, outputs rounded to the
kernel's dtype) stays inside them on EVERY case of both tables, and every mutant of norm_ref.MUTANTS leaves them on a named case.

Which case kills which mutant (the tensor that leaves its bound; `[mutant]` lines of this module print the shares):
  one_pass_var       fwd-hard-9-264-mean300 f32   rstd, y     (E[x^2] ~ 9e4 in float32 loses the variance 2.5e-3; random rows pass)
  unbiased_ln_var    fwd-width-5-264-randn        rstd, y
  eps_outside        fwd-hard-9-264-const_eps5    rstd        (1 / eps instead of 1 / sqrt(eps); y = beta either way)
  tail8              fwd-width-5-264-randn        mean, rstd, y   (columns 256 .. 263: the whole second chunk of N = 264)
  last_row           fwd-rows-9-264-randn         y;  bwd-rows-9-264-randn   dx, dgamma, dbeta
  dx_no_s2           bwd-width-9-264-randn        dx
  dx_no_dres         bwd-width-9-264-randn        dx
  dgamma_gdy         bwd-width-9-264-randn        dgamma
  overwrite          bwd-width-9-264-randn        dgamma, dbeta;  bn bwd-7-264-randn  dgamma, dbeta   (non-zero start values)
  bn_biased_running  stats-2-264-randn            run_var     (a factor 2 at M = 2; 1 / 128 at M = 129)
  bn_no_m1           bwd-7-264-randn              dy
  swish_no_x         bwd-7-264-randn              dy, dgamma, dbeta and both means
  last_row           stats-129-264-randn          var, run_var;  bn bwd-7-264-randn   every output"""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as R

F64 = torch.float64
DTYPES = ["f32", "bf16"]


def _close(a, b, tol=1e-11):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---- the float64 reference is torch's ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,eps", [(5, 12, 1e-5), (9, 264, 1e-12), (33, 1020, 1e-5)])
def test_layernorm_reference_is_torch_autograd(M, N, eps):
    g = torch.Generator().manual_seed(M * N)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x, gamma, beta, dy, dres = rn(M, N) * 2 + 0.5, 1 + 0.3 * rn(N), rn(N), rn(M, N), rn(M, N)
    leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta)]
    want = F.layer_norm(leaves[0], (N,), leaves[1], leaves[2], eps)
    (want * dy).sum().backward()
    y, mean, rstd = R.ln_fwd(x, gamma, beta, eps)
    assert _close(y, want.detach()) and _close(mean, x.mean(1)) and _close(rstd, (x.var(1, unbiased=False) + eps).rsqrt())
    dx, dgamma, dbeta, ag, ab = R.ln_bwd(dy, x, gamma, mean, rstd, dres)
    assert _close(dx, leaves[0].grad + dres) and _close(dgamma, leaves[1].grad) and _close(dbeta, leaves[2].grad)
    assert _close(R.ln_bwd(dy, x, gamma, mean, rstd, None)[0], leaves[0].grad)
    xh = (x - mean[:, None]) * rstd[:, None]
    assert _close(ag, (dy * xh).abs().sum(0)) and _close(ab, dy.abs().sum(0))


@pytest.mark.parametrize("M,C", [(2, 8), (17, 12), (129, 264)])
def test_batchnorm_swish_reference_is_torch_autograd(M, C):
    g = torch.Generator().manual_seed(M * C)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    y, gamma, beta, dz, rm0, rv0 = rn(M, C) * 1.5 + 0.3, 1 + 0.3 * rn(C), rn(C), rn(M, C), rn(C), rn(C).abs() + 0.5
    leaves = [t.clone().requires_grad_(True) for t in (y, gamma, beta)]
    rm, rv = rm0.clone(), rv0.clone()
    want = F.silu(F.batch_norm(leaves[0], rm, rv, leaves[1], leaves[2], training=True, momentum=0.1, eps=1e-5))
    (want * dz).sum().backward()
    mean, var, rm1, rv1 = R.bn_stats(y, rm0, rv0, 0.1)
    assert _close(mean, y.mean(0)) and _close(var, y.var(0, unbiased=False)) and _close(rm1, rm) and _close(rv1, rv)
    assert _close(R.bn_swish_fwd(y, mean, var, gamma, beta, 1e-5), want.detach())
    dy, dgamma, dbeta, m1, m2, ag, ab = R.bn_swish_bwd(dz, y, mean, var, gamma, beta, 1e-5)
    assert _close(dy, leaves[0].grad) and _close(dgamma, leaves[1].grad) and _close(dbeta, leaves[2].grad)
    assert _close(m1, dbeta / M) and _close(m2, dgamma / M) and bool((ag >= dgamma.abs() - 1e-12).all()) and bool((ab >= dbeta.abs() - 1e-12).all())


def test_one_row_of_batchnorm_takes_the_biased_variance_into_the_running_one():
    y, rm0, rv0 = torch.tensor([[1.5, -2.0]], dtype=F64), torch.zeros(2, dtype=F64), torch.ones(2, dtype=F64)
    mean, var, rm, rv = R.bn_stats(y, rm0, rv0, 0.1)
    assert torch.equal(mean, y[0]) and torch.equal(var, torch.zeros(2, dtype=F64))
    assert _close(rm, 0.1 * y[0]) and _close(rv, torch.full((2,), 0.9, dtype=F64))


# ---- the bounds admit a correct float32 implementation: every case of both tables ------------------------------------------------------
def _show(tag, case, res):
    print(f"[{tag}] norm {R.case_id(case)}: " + ", ".join(f"{k} {v:.2f}" for k, v in res.items()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.LN_CASES, ids=R.case_id)
def test_model_of_layernorm_is_inside_the_bounds(case, dtype):
    inp = R.ln_inputs(case, R.dtype_of(dtype))
    if case[0] == "fwd":
        y, mean, rstd = R.model_ln_fwd(inp)
        res = R.check_ln_fwd(inp, y, mean, rstd)
        if case[4].startswith("const"):      # (the case is what it claims to be: zero variance, y = beta)
            assert float(rstd.min()) > 0.99 * inp.eps ** -0.5 and bool((y.double() - inp.beta.double()).abs().max() <= 2 ** -8 * 2)
    else:
        res = R.check_ln_bwd(inp, *R.model_ln_bwd(inp))
        res.update({k + "/no_dres": v for k, v in R.check_ln_bwd(inp, R.model_ln_bwd(inp, dres=False)[0], dres=False).items()})
    _show("model", case, res)
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.BN_STATS_CASES + R.BN_FWD_CASES + R.BN_BWD_CASES, ids=R.case_id)
def test_model_of_batchnorm_swish_is_inside_the_bounds(case, dtype):
    inp = R.bn_inputs(case, R.dtype_of(dtype))
    if case[0] == "stats":
        res = R.check_bn_stats(inp, *R.model_bn_stats(inp))
    elif case[0] == "fwd":
        res = R.check_bn_fwd(inp, R.model_bn_fwd(inp))
    else:
        res = R.check_bn_bwd(inp, *R.model_bn_bwd(inp))
    _show("model", case, res)
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("case,dtype", list(zip(R.BN_FWD_BIG_CASES, ["bf16", "f32"])), ids=str)
def test_model_of_the_grid_stride_cases_is_inside_the_bounds(case, dtype):
    inp = R.bn_inputs(case, R.dtype_of(dtype))
    assert inp.M * inp.C // (8 if inp.C % 8 == 0 else 1) > 8192 * 256
    res = R.check_bn_fwd(inp, R.model_bn_fwd(inp))
    _show("model", case, res)
    assert max(res.values()) <= 1.0, res


def test_hard_cases_are_what_they_claim():
    inp = R.bn_inputs(("fwd", 17, 264, "sat"), torch.float32)
    bn = R._bn(*[t.double() for t in (inp.y, inp.mean, inp.var, inp.gamma, inp.beta)], inp.eps)[1]
    assert float(bn.abs().min()) > 19.5 and bool((bn > 0).any()) and bool((bn < 0).any())
    inp = R.bn_inputs(("fwd", 17, 264, "near0"), torch.float32)
    bn = R._bn(*[t.double() for t in (inp.y, inp.mean, inp.var, inp.gamma, inp.beta)], inp.eps)[1]
    assert float(bn.abs().max()) < 1e-2
    for dt in (torch.float32, torch.bfloat16):
        inp = R.bn_inputs(("bwd", 17, 264, "zero_var"), dt)
        assert bool((inp.var[::3] == 0).all()) and bool((inp.var[1::3] > 0.1).all())
        inp = R.ln_inputs(("fwd", "hard", 9, 1020, "const_eps12", 1e-12), dt)
        assert float(inp.rstd.min()) > 0.99e6 and bool((inp.x.var(1) == 0).all())


# ---- the bounds reject a wrong kernel: each mutant on a named case ------------------------------------------------------------------------
_W, _R9, _H = ("fwd", "width", 5, 264, "randn", 1e-5), ("fwd", "rows", 9, 264, "randn", 1e-12), ("bwd", "width", 9, 264, "randn", 64)
_LN_MUTANTS = [
    ("one_pass_var", ("fwd", "hard", 9, 264, "mean300", 1e-5), "f32", ("rstd", "y")),
    ("unbiased_ln_var", _W, "bf16", ("rstd", "y")),
    ("eps_outside", ("fwd", "hard", 9, 264, "const_eps5", 1e-5), "bf16", ("rstd",)),
    ("tail8", _W, "bf16", ("mean", "rstd", "y")),
    ("last_row", _R9, "bf16", ("y",)),
    ("last_row", ("bwd", "rows", 9, 264, "randn", 64), "bf16", ("dx", "dgamma", "dbeta")),
    ("dx_no_s2", _H, "bf16", ("dx",)),
    ("dx_no_dres", _H, "bf16", ("dx",)),
    ("dgamma_gdy", _H, "bf16", ("dgamma",)),
    ("overwrite", _H, "f32", ("dgamma", "dbeta")),
]
_BN_MUTANTS = [
    ("bn_biased_running", ("stats", 2, 264, "randn"), "f32", ("run_var",)),
    ("bn_biased_running", ("stats", 129, 264, "randn"), "f32", ("run_var",)),
    ("last_row", ("stats", 129, 264, "randn"), "f32", ("var", "run_var")),
    ("bn_no_m1", ("bwd", 7, 264, "randn"), "bf16", ("dy",)),
    ("swish_no_x", ("bwd", 7, 264, "randn"), "bf16", ("dy", "dgamma", "dbeta", "m1", "m2")),
    ("overwrite", ("bwd", 7, 264, "randn"), "f32", ("dgamma", "dbeta")),
    ("last_row", ("bwd", 7, 264, "randn"), "f32", ("dy", "dgamma", "dbeta", "m1", "m2")),
]
_mid = lambda v: R.case_id(v) if isinstance(v, tuple) and v[0] in ("fwd", "bwd", "stats") else "+".join(v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("mutant,case,dtype,hit", _LN_MUTANTS, ids=_mid)
def test_layernorm_mutants_leave_the_bounds(mutant, case, dtype, hit):
    assert case in R.LN_CASES and mutant in R.MUTANTS
    inp = R.ln_inputs(case, R.dtype_of(dtype))
    res = R.check_ln_fwd(inp, *R.model_ln_fwd(inp, mutant)) if case[0] == "fwd" else R.check_ln_bwd(inp, *R.model_ln_bwd(inp, mutant))
    _show(f"mutant {mutant}", case, res)
    for k in hit:
        assert res[k] > 1.0, (k, res)
    for k in set(res) - set(hit):      # (and nothing else moves)
        assert res[k] <= 1.0, (k, res)


@pytest.mark.parametrize("mutant,case,dtype,hit", _BN_MUTANTS, ids=_mid)
def test_batchnorm_swish_mutants_leave_the_bounds(mutant, case, dtype, hit):
    assert case in R.BN_CASES and mutant in R.MUTANTS
    inp = R.bn_inputs(case, R.dtype_of(dtype))
    res = (R.check_bn_stats(inp, *R.model_bn_stats(inp, mutant)) if case[0] == "stats"
           else R.check_bn_bwd(inp, *R.model_bn_bwd(inp, mutant)))
    _show(f"mutant {mutant}", case, res)
    for k in hit:
        assert res[k] > 1.0, (k, res)
    for k in set(res) - set(hit):
        assert res[k] <= 1.0, (k, res)


def test_every_mutant_of_the_table_is_killed_somewhere():
    assert {m for m, *_ in _LN_MUTANTS + _BN_MUTANTS} == set(R.MUTANTS) - {None}


def test_one_pass_variance_passes_on_the_easy_inputs():
    """why the hard cases exist: on randn * 2 + 0.5, the only distribution the older tests use, E[x^2] - E[x]^2 is inside every bound"""
    inp = R.ln_inputs(("fwd", "width", 5, 264, "randn", 1e-5), torch.float32)
    res = R.check_ln_fwd(inp, *R.model_ln_fwd(inp, "one_pass_var"))
    assert max(res.values()) <= 1.0, res
