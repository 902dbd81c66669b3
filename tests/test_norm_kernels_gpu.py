"""The LayerNorm kernels of csrc/layernorm.hip and the BatchNorm + Swish kernels of csrc/convmodule.hip against the float64
restatement of tests/norm_ref.py (pinned on the CPU by tests/test_norm_ref_cpu.py), through the C ABI with the test's own buffers:
every output is NaN-filled with a 64-element NaN guard behind it (after the launch every defined element is finite, the guard
untouched), dgamma / dbeta start from non-zero random values (the expectation is start + reference), options are set by
lib.options scopes only.  Bounds: tests/norm_ref.py (element outputs, statistics, the order-independent column-sum bound; none
taken from the kernels).

PATH COVERAGE, from the dispatch conditions (ids of norm_ref.LN_CASES / BN_CASES; every id runs in f32 and bf16):
  emoasr_layernorm_fwd: M <= 4096 -> ln_fwd_kernel<T, true>; else N % 8 == 0 and option ln_fwd8 -> ln_fwd8_kernel<T, cdiv(N, 256)>;
  else ln_fwd_kernel<T, false>
    ln_fwd_kernel<., true>     fwd-width-5-*  fwd-rows-{1,3,4,5,7,8,9,4096}-{264,1020}  fwd-hard-9-*
    ln_fwd_kernel<., false>    fwd-width-4097-{4,12,252,260,1020}  fwd-rows-{4097,4099,4104}-1020  (N % 4 only), and every
                               M > 4096 case of N % 8 == 0 under ln_fwd8 = 0
    ln_fwd8_kernel NC = 1      fwd-width-4097-{8,64,144,248,256}
                   NC = 2      fwd-width-4097-{264,504,512}  fwd-rows-{4097,4099,4104}-264
                   NC = 3      fwd-width-4097-{520,768}
                   NC = 4      fwd-width-4097-{1016,1024}
  emoasr_layernorm_bwd_ex: N % 8 == 0 -> ln_bwd8_kernel<T, cdiv(N, 256), PF = option ln_bwd_pf and nblk * 8 < M>,
  nblk = min(cdiv(M, 8), option ln_bwd_blocks); else ln_bwd_kernel<T>, nblk = min(cdiv(M, 4), 256); each case under ln_bwd_pf = 1, 0
    ln_bwd_kernel              bwd-width-{5,1029}-{4,12,252,260,1020}  bwd-rows-{1,4,5,1024,1025,1029}-{260,1020}
                               bwd-hard-9-1020-*; with `branch`: test_layernorm_bwd_arguments[general-*]
    ln_bwd8_kernel NC = 1      PF on: bwd-width-519-{8..256} (65 rows at 64 blocks)   PF off: the same under ln_bwd_pf = 0,
                               bwd-width-9-{8..256}, bwd-finalize-*-72
                   NC = 2      PF on: bwd-width-519-{264,504,512}  bwd-trips-{513,519,1024,1029,4097}-264
                               PF off: bwd-trips-512-264 (nblk * 8 = M), bwd-rows-{1,7,8,9}-264, bwd-hard-9-264-*, and ln_bwd_pf = 0
                   NC = 3      PF on: bwd-width-519-{520,768}      PF off: bwd-width-9-{520,768} and ln_bwd_pf = 0
                   NC = 4      PF on: bwd-width-519-{1016,1024}  bwd-trips-{513,519,1024,1029,4097}-1024
                               PF off: bwd-trips-512-1024, bwd-width-9-{1016,1024} and ln_bwd_pf = 0
    ln_bwd_finalize_kernel     every bwd case (gridDim.y 1 .. 8: bwd-finalize-{8,248,256,264,520,2040,2048,4096}-72)
    ln_bwd_finalize_grouped_kernel   test_layernorm_bwd_grouped_finalize (six items: N 8 .. 1024, nblk 2 .. 256, one dgamma-only, one
                               dbeta-only)
  emoasr_bn_swish_fwd: C % 8 == 0 and y, z 16-byte aligned -> bn_swish_fwd8_kernel; else bn_swish_fwd_kernel
    bn_swish_fwd8_kernel       fwd-*-{8,144,256,264}-*, second grid-stride trip: fwd-2097155-8-randn (bf16)
    bn_swish_fwd_kernel        fwd-*-12-*, test_bn_swish_fwd_misaligned_view, second trip: fwd-174763-12-randn (f32)
  emoasr_bn_stats              bn_sum / bn_var / bn_finalize_kernel: stats-* (M on both sides of 64 and 128, C on both sides of 256)
  emoasr_bn_swish_bwd(_sums)   bn_bwd_sums / fold / apply_kernel: bwd-* (65 partial rows: bwd-4097-*), test_bn_swish_bwd_sums_alone
  emoasr_bn_stats_finalize     bn_stats_finalize_kernel: conv-* (140 partial blocks: conv-70-33-24-31; 64 channel groups: conv-2-33-1024-7)

MEASURED on an MI355X, worst share of the bound per family (the `[measured] norm <family>` lines this module prints when it is
done; f32 | bf16):
  ln_fwd     width       y 0.250, mean 0.129, rstd 0.064 | y 0.995, mean 0.056, rstd 0.098    (ln_fwd8 = 0: the same to 0.03)
             rows        y 0.127, mean 0.046, rstd 0.045 | y 0.995, mean 0.055, rstd 0.050
             hard        y 0.115, mean 0.100, rstd 0.066 | y 0.988, mean 0.046, rstd 0.078
  ln_bwd     width       dx 0.250, dgamma 0.148, dbeta 0.116 | dx 0.995, dgamma 0.131, dbeta 0.044
             trips       dx 0.201, dgamma 0.001, dbeta 0.001 | dx 0.996, dgamma 0.001, dbeta 0.000
             rows        dx 0.210, dgamma 0.122, dbeta 0.094 | dx 0.996, dgamma 0.119, dbeta 0.046
             finalize    dx 0.234, dgamma 0.071, dbeta 0.056 | dx 0.995, dgamma 0.082, dbeta 0.024
             hard        dx 0.209, dgamma 0.117, dbeta 0.090 | dx 0.989, dgamma 0.099, dbeta 0.033
             arguments   dx 0.143, dgamma 0.001, dbeta 0.000 | dx 0.996, dgamma 0.001, dbeta 0.000   (both kernels)
             grouped     dx 0.197, dgamma 0.040, dbeta 0.077, against the immediate fold 0.052 | dx 0.996, 0.046, 0.033, 0.027
  bn_stats   randn       mean 0.194, var 0.250, run_mean 0.091, run_var 0.095 | mean 0.036, var 0.250, run_mean 0.085, run_var 0.083
             mean50      mean 0.139, var 0.000, run_mean 0.113, run_var 0.054 | all <= 0.059 (50 +- 0.01 is the constant 50 in bf16)
  bn_swish_fwd           randn z 0.202 | 0.994   sat 0.047 | 0.662   near0 0.000 | 0.857   zero_var 0.168 | 0.982
                         grid stride z 0.222 (f32, element-wise form) | 0.991 (bf16, 8-wide form)
  bn_swish_bwd randn     dy 0.290, dgamma 0.143, dbeta 0.176, m1 0.101, m2 0.074 | dy 0.995, dgamma 0.145, dbeta 0.133, m1 0.101, m2 0.099
             sat         dy 0.005, sums <= 0.054 | dy 0.947, sums <= 0.072      near0  dy 0.000, sums <= 0.060 | dy 0.848, sums <= 0.076
             zero_var    dy 0.158, sums <= 0.075 | dy 0.969, sums <= 0.085      sums alone  <= 0.124 | <= 0.115
  bn_stats_finalize      mean 0.126, var 0.168, run_mean 0.070, run_var 0.066 | mean 0.101, var 0.112, run_mean 0.070, run_var 0.063
Every share near 1 is a bf16 ELEMENT output (y, dx, z, dy): the term of its bound that is reached is 2^-8 |ref|, bf16's worst
rounding, which is the bound by construction (the f32 column beside it shows the arithmetic before that rounding at a quarter of its
bound or less).  The statistics and the column sums sit at a quarter of their bounds or less in both dtypes; a column sum over 4097
rows uses a thousandth of the order-independent term.  The 0.250 entries are cases whose bound is 4 e32: the kernel and the float32
model are one rounding apart from the reference at the same element.

What the sweep exposed: nothing.  Every kernel template of both files, on every path listed above, held every bound, every
bit-identity (ln_bwd_pf on / off, with / without statistics, parameter gradients, branch, defer_finalize, the two BatchNorm forward
forms), every NaN guard and every refusal.  That the module can fail was tried on a scratch build with three in-bounds errors
planted, none of which the LayerNorm / BatchNorm tests of test_ops_gpu.py see: the prefetch of ln_bwd8_kernel issued before the
current row is unpacked (fails the 44 multi-trip cases of test_layernorm_bwd, the half_wave arguments test and the grouped fold), a
fold that stores dgamma where it runs a single slice (the 86 cases of fewer than 64 blocks), bn_bwd_fold_kernel without its second
trip (the six M = 4097 cases)."""
import ctypes

import pytest
import torch

from tests import norm_ref as R

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
DTYPES = ["f32", "bf16"]


def _nan_out(dev, shape, dtype):
    """a NaN-filled tensor of this shape with 64 NaN guard elements behind it -> (tensor, guard)"""
    n = 1
    for v in shape:
        n *= v
    flat = torch.full((n + 64,), NAN, device=dev, dtype=dtype)
    return flat[:n].view(*shape), flat[n:]


def _untouched(*guards):
    return all(bool(torch.isnan(g).all()) for g in guards)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _code(dtype):
    from emoasr_amd import lib
    return lib.BF16 if dtype == BF else lib.F32


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cpu(t):
    return None if t is None else t.detach().to("cpu", F32)


_WORST = {}      # family -> dtype -> tensor -> worst share of the bound over the family's cases


def _report(family, dtype, case, res):
    """every case must be inside its bounds; the worst shares are kept per family and dtype and printed once, when the module is done"""
    w = _WORST.setdefault(family, {}).setdefault(dtype, {})
    for k, v in res.items():
        w[k] = max(v, w.get(k, 0.0))
    assert max(res.values()) <= 1.0, (family, dtype, case, res)


@pytest.fixture(scope="module", autouse=True)
def _measured():
    yield
    for family, by_dtype in _WORST.items():
        print(f"\n[measured] norm {family}: " + " | ".join(dt + " " + ", ".join(f"{k} {v:.3f}" for k, v in w.items())
                                                            for dt, w in by_dtype.items()), end="")
    print()


def _up(dev, t, dtype=F32):
    return None if t is None else t.to(dtype).to(dev)


# ---- launches on the test's own buffers ---------------------------------------------------------------------------------------------
def _ln_fwd(dev, x, gamma, beta, eps, stats=True):
    """-> y, mean, rstd (None without stats), guards"""
    from emoasr_amd import lib
    M, N = x.shape
    y, g0 = _nan_out(dev, (M, N), x.dtype)
    (mean, g1), (rstd, g2) = (_nan_out(dev, (M,), F32), _nan_out(dev, (M,), F32)) if stats else ((None, g0), (None, g0))
    lib.call("emoasr_layernorm_fwd", _code(x.dtype), M, N, _p(x), _p(gamma), _p(beta), eps, _p(y), _p(mean), _p(rstd), _stream())
    return y, mean, rstd, (g0, g1, g2)


def _ln_bwd(dev, d, dres=True, dgamma=None, dbeta=None, branch=None, deferred=None):
    """d: the device tensors of one case; dgamma / dbeta: the buffers to accumulate into -> dx, dy_branch, guards"""
    from emoasr_amd import lib
    M, N = d.x.shape
    dx, g0 = _nan_out(dev, (M, N), d.x.dtype)
    dy2, g1 = _nan_out(dev, (M, N), d.x.dtype) if branch is not None else (None, g0)
    scratch = None
    if dgamma is not None or dbeta is not None:
        scratch = torch.empty(lib.size_query("emoasr_layernorm_bwd_scratch_floats", N), device=dev, dtype=F32)
    o = lib.LnBwdOpts()
    if branch is not None:
        o.dy2, o.scale2, o.drop_p2, o.seed2 = dy2.data_ptr(), branch[0], branch[1], branch[2]
    if deferred is not None and scratch is not None:
        o.defer_finalize = 1
        deferred.append((M, N, scratch, dgamma, dbeta))
    lib.call("emoasr_layernorm_bwd_ex", _code(d.x.dtype), M, N, _p(d.dy), _p(d.x), _p(d.gamma), _p(d.mean), _p(d.rstd),
             _p(d.dres if dres else None), _p(dx), _p(dgamma), _p(dbeta), _p(scratch), ctypes.byref(o), _stream())
    return dx, dy2, (g0, g1)


def _ln_dev(dev, inp):
    from types import SimpleNamespace
    dt = inp.dtype
    return SimpleNamespace(x=_up(dev, inp.x, dt), dy=_up(dev, inp.dy, dt), dres=_up(dev, inp.dres, dt), gamma=_up(dev, inp.gamma),
                           beta=_up(dev, inp.beta), mean=_up(dev, inp.mean), rstd=_up(dev, inp.rstd))


def _acc_bufs(dev, inp):
    """dgamma / dbeta holding their start values, each with a NaN guard behind it"""
    n = inp.dg0.numel()
    (dg, g0), (db, g1) = _nan_out(dev, (n,), F32), _nan_out(dev, (n,), F32)
    dg.copy_(inp.dg0)
    db.copy_(inp.db0)
    return dg, db, (g0, g1)


# ---- LayerNorm forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.LN_FWD_CASES, ids=R.case_id)
def test_layernorm_fwd(dev, case, dtype):
    """under ln_fwd8 = 1 and 0 (two kernels for N % 8 == 0 and M > 4096: each held to the reference, not to each other -- their
    summation orders differ); without statistics y is bit-identical"""
    from emoasr_amd import lib
    inp = R.ln_inputs(case, R.dtype_of(dtype))
    d = _ln_dev(dev, inp)
    for fwd8 in (1, 0):
        with lib.options(ln_fwd8=fwd8):
            y, mean, rstd, guards = _ln_fwd(dev, d.x, d.gamma, d.beta, inp.eps)
            y0, _, _, guards0 = _ln_fwd(dev, d.x, d.gamma, d.beta, inp.eps, stats=False)
        torch.cuda.synchronize()
        assert _untouched(*guards, *guards0), "a store behind an output"
        assert torch.equal(y0, y), "y depends on whether the statistics are asked for"
        res = R.check_ln_fwd(inp, _cpu(y), _cpu(mean), _cpu(rstd))
        if case[4].startswith("const"):      # zero variance: rstd = 1 / sqrt(eps), y = beta (+ its bf16 rounding)
            assert float(rstd.min()) > 0.99 * inp.eps ** -0.5
        _report(f"ln_fwd {case[1]}" + ("" if fwd8 else " ln_fwd8=0"), dtype, case, res)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [2, 1028])
def test_layernorm_refuses_unsupported_widths(dev, N, dtype):
    from emoasr_amd import lib
    M, dt = 5, R.dtype_of(dtype)
    x, gamma = torch.zeros(M, N, device=dev, dtype=dt), torch.ones(N, device=dev)
    y, gy = _nan_out(dev, (M, N), dt)
    mean, gm = _nan_out(dev, (M,), F32)
    with pytest.raises(lib.EmoasrHipError, match="unsupported"):
        lib.call("emoasr_layernorm_fwd", _code(dt), M, N, _p(x), _p(gamma), _p(gamma), 1e-5, _p(y), _p(mean), _p(mean), _stream())
    dx, gx = _nan_out(dev, (M, N), dt)
    with pytest.raises(lib.EmoasrHipError, match="unsupported"):
        lib.call("emoasr_layernorm_bwd", _code(dt), M, N, _p(x), _p(x), _p(gamma), _p(gamma), _p(gamma), None, _p(dx), None, None,
                 None, _stream())
    torch.cuda.synchronize()
    for t in (y, gy, mean, gm, dx, gx):
        assert bool(torch.isnan(t).all())


# ---- LayerNorm backward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.LN_BWD_CASES, ids=R.case_id)
def test_layernorm_bwd(dev, case, dtype):
    """every trip pattern of the half-wave walk (norm_ref.LN_BWD_TRIPS) under ln_bwd_pf = 1 and 0: prefetch changes when the loads
    issue, not the arithmetic -- dx agrees bit for bit, and both runs are held to the reference"""
    from emoasr_amd import lib
    inp = R.ln_inputs(case, R.dtype_of(dtype))
    d = _ln_dev(dev, inp)
    dxs = []
    with lib.options(ln_bwd_blocks=case[5]):
        for pf in (1, 0):
            with lib.options(ln_bwd_pf=pf):
                dg, db, ga = _acc_bufs(dev, inp)
                dx, _, guards = _ln_bwd(dev, d, dgamma=dg, dbeta=db)
                torch.cuda.synchronize()
            assert _untouched(*guards, *ga), "a store behind an output"
            _report(f"ln_bwd {case[1]}", dtype, case, R.check_ln_bwd(inp, _cpu(dx), _cpu(dg), _cpu(db)))
            dxs.append(dx)
    assert torch.equal(dxs[0], dxs[1]), "dx depends on ln_bwd_pf"


_ARG_CASES = {"half_wave": ("bwd", "trips", 519, 264, "randn", 64), "general": ("bwd", "rows", 1029, 260, "randn", 64)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", list(_ARG_CASES))
def test_layernorm_bwd_arguments(dev, kernel, dtype):
    """dres present / None x (dgamma and dbeta | dgamma | dbeta | neither): each held to the reference, an absent one not needed;
    with neither, dx is bit-identical to the run with both.  branch = (scale, p, seed): dy_branch is ops.scale_dropout of the stored
    dx bit for bit, and dx is bit-identical to the run without it."""
    from emoasr_amd import lib, ops
    case = _ARG_CASES[kernel]
    assert case in R.LN_BWD_CASES
    inp = R.ln_inputs(case, R.dtype_of(dtype))
    d = _ln_dev(dev, inp)
    with lib.options(ln_bwd_blocks=case[5]):
        for dres in (True, False):
            both = None
            for want_g, want_b in ((True, True), (True, False), (False, True), (False, False)):
                dg, db, ga = _acc_bufs(dev, inp)
                dx, _, guards = _ln_bwd(dev, d, dres=dres, dgamma=dg if want_g else None, dbeta=db if want_b else None)
                torch.cuda.synchronize()
                assert _untouched(*guards, *ga), "a store behind an output"
                res = R.check_ln_bwd(inp, _cpu(dx), _cpu(dg) if want_g else None, _cpu(db) if want_b else None, dres=dres)
                _report(f"ln_bwd arguments {kernel}", dtype, (case, dres, want_g, want_b), res)
                if not want_g:
                    assert torch.equal(dg.cpu(), inp.dg0), "dgamma written though not asked for"
                if not want_b:
                    assert torch.equal(db.cpu(), inp.db0), "dbeta written though not asked for"
                both = dx if both is None else both
                assert torch.equal(dx, both), "dx depends on which parameter gradients are asked for"
            if dres:
                dg, db, ga = _acc_bufs(dev, inp)
                dxb, dyb, guards = _ln_bwd(dev, d, dgamma=dg, dbeta=db, branch=(0.5, 0.1, 77))
                torch.cuda.synchronize()
                assert _untouched(*guards, *ga), "a store behind an output"
                assert torch.equal(dxb, both), "dx depends on the branch output"
                assert torch.equal(dyb, ops.scale_dropout(both.contiguous(), 0.5, 0.1, 77)), "dy_branch is not scale_dropout(dx)"
                assert 0.05 < float((dyb == 0).float().mean()) < 0.2      # (the dropout did drop)
                _report(f"ln_bwd arguments {kernel}", dtype, (case, "branch"), R.check_ln_bwd(inp, _cpu(dxb), _cpu(dg), _cpu(db)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_bwd_grouped_finalize(dev, dtype):
    """one grouped fold over items that differ in N and nblk (the grid follows the widest and the deepest), one dgamma-only and one
    dbeta-only.  ONE options scope spans the deferred backwards and the fold: the fold reads ln_bwd_blocks again.  Before the fold
    dgamma / dbeta are their start values bit for bit; after it each is within the column-sum bound of its own immediate fold and of
    the reference."""
    from emoasr_amd import lib, ops
    items = [(("bwd", "width", 9, 8, "randn", 64), True, True), (("bwd", "trips", 4097, 1024, "randn", 512), True, True),
             (("bwd", "trips", 513, 264, "randn", 64), True, True), (("bwd", "rows", 1029, 260, "randn", 64), True, True),
             (("bwd", "trips", 519, 264, "randn", 64), True, False), (("bwd", "rows", 7, 264, "randn", 64), False, True)]
    deferred, held = [], []
    with lib.options(ln_bwd_blocks=64):
        for case, want_g, want_b in items:
            assert case in R.LN_BWD_CASES
            inp = R.ln_inputs(case, R.dtype_of(dtype))
            d = _ln_dev(dev, inp)
            dg_i, db_i, ga_i = _acc_bufs(dev, inp)
            dx_i, _, gi = _ln_bwd(dev, d, dgamma=dg_i if want_g else None, dbeta=db_i if want_b else None)
            dg, db, ga = _acc_bufs(dev, inp)
            dx, _, gd = _ln_bwd(dev, d, dgamma=dg if want_g else None, dbeta=db if want_b else None, deferred=deferred)
            torch.cuda.synchronize()
            assert torch.equal(dx, dx_i), "dx depends on defer_finalize"
            assert torch.equal(dg.cpu(), inp.dg0) and torch.equal(db.cpu(), inp.db0), "folded before the finalize"
            held.append((case, inp, want_g, want_b, dx, dg, db, dg_i, db_i, ga + ga_i + gi + gd))
        assert len(deferred) == len(items)
        ops.layernorm_bwd_finalize(deferred)
        torch.cuda.synchronize()
    for case, inp, want_g, want_b, dx, dg, db, dg_i, db_i, guards in held:
        assert _untouched(*guards), "a store behind an output"
        res = R.check_ln_bwd(inp, _cpu(dx), _cpu(dg) if want_g else None, _cpu(db) if want_b else None)
        ref = R.eval_ln_bwd(inp, R.F64)
        m32 = R.eval_ln_bwd(inp, R.F32)
        for name, on, got, imm, k, start in (("dgamma", want_g, dg, dg_i, 1, inp.dg0), ("dbeta", want_b, db, db_i, 2, inp.db0)):
            if on:
                bound = R.colsum_bound(start.double() + ref[k], start + m32[k], inp.M, ref[k + 2])
                res[name + " vs immediate"] = float(((got.cpu().double() - imm.cpu().double()).abs() / bound).max())
            else:
                assert torch.equal(got.cpu(), start), f"{name} written though not asked for"
        _report("ln_bwd grouped finalize", dtype, case, res)


# ---- BatchNorm statistics -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.BN_STATS_CASES, ids=R.case_id)
def test_bn_stats(dev, case, dtype):
    from emoasr_amd import lib
    inp = R.bn_inputs(case, R.dtype_of(dtype))
    y = _up(dev, inp.y, inp.dtype)
    (mean, g0), (var, g1), (rm, g2), (rv, g3) = (_nan_out(dev, (inp.C,), F32) for _ in range(4))
    rm.copy_(inp.rm0)
    rv.copy_(inp.rv0)
    lib.call("emoasr_bn_stats", _code(inp.dtype), inp.M, inp.C, _p(y), _p(mean), _p(var), _p(rm), _p(rv), inp.momentum, _stream())
    torch.cuda.synchronize()
    assert _untouched(g0, g1, g2, g3), "a store behind an output"
    _report(f"bn_stats {case[3]}", dtype, case, R.check_bn_stats(inp, _cpu(mean), _cpu(var), _cpu(rm), _cpu(rv)))
    # without running statistics: the same mean / var bit for bit
    (mean1, g4), (var1, g5) = _nan_out(dev, (inp.C,), F32), _nan_out(dev, (inp.C,), F32)
    lib.call("emoasr_bn_stats", _code(inp.dtype), inp.M, inp.C, _p(y), _p(mean1), _p(var1), None, None, inp.momentum, _stream())
    torch.cuda.synchronize()
    assert _untouched(g4, g5)
    if inp.M <= 64:      # (one block per column: no atomics between blocks, so the order is fixed)
        assert torch.equal(mean1, mean) and torch.equal(var1, var)
    _report(f"bn_stats {case[3]}", dtype, case, {k: v for k, v in R.check_bn_stats(inp, _cpu(mean1), _cpu(var1), _cpu(rm), _cpu(rv)).items()
                                          if k in ("mean", "var")})


# ---- BatchNorm + Swish forward --------------------------------------------------------------------------------------------------------
def _bn_dev(dev, inp):
    from types import SimpleNamespace
    return SimpleNamespace(y=_up(dev, inp.y, inp.dtype), dz=_up(dev, inp.dz, inp.dtype), mean=_up(dev, inp.mean), var=_up(dev, inp.var),
                           gamma=_up(dev, inp.gamma), beta=_up(dev, inp.beta))


def _bn_fwd(dev, inp, d, y=None, z=None):
    from emoasr_amd import lib
    guard = None
    if z is None:
        z, guard = _nan_out(dev, (inp.M, inp.C), inp.dtype)
    lib.call("emoasr_bn_swish_fwd", _code(inp.dtype), inp.M, inp.C, _p(d.y if y is None else y), _p(d.mean), _p(d.var), _p(d.gamma),
             _p(d.beta), inp.eps, _p(z), _stream())
    return z, guard


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.BN_FWD_CASES, ids=R.case_id)
def test_bn_swish_fwd(dev, case, dtype):
    inp = R.bn_inputs(case, R.dtype_of(dtype))
    z, guard = _bn_fwd(dev, inp, _bn_dev(dev, inp))
    torch.cuda.synchronize()
    assert _untouched(guard), "a store behind an output"
    _report(f"bn_swish_fwd {case[3]}", dtype, case, R.check_bn_fwd(inp, _cpu(z)))


@pytest.mark.parametrize("case,dtype", list(zip(R.BN_FWD_BIG_CASES, ["bf16", "f32"])), ids=str)
def test_bn_swish_fwd_second_grid_stride_trip(dev, case, dtype):
    inp = R.bn_inputs(case, R.dtype_of(dtype))
    assert inp.M * inp.C // (8 if inp.C % 8 == 0 else 1) > 8192 * 256
    z, guard = _bn_fwd(dev, inp, _bn_dev(dev, inp))
    torch.cuda.synchronize()
    assert _untouched(guard), "a store behind an output"
    _report("bn_swish_fwd grid stride", dtype, case, R.check_bn_fwd(inp, _cpu(z)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 264])
def test_bn_swish_fwd_misaligned_view(dev, C, dtype):
    """y and z 8 bytes off a 16-byte boundary take the element-wise form, which promises the 8-wide form's results bit for bit"""
    case = ("fwd", 17, C, "randn")
    assert case in R.BN_FWD_CASES
    inp = R.bn_inputs(case, R.dtype_of(dtype))
    d = _bn_dev(dev, inp)
    z, guard = _bn_fwd(dev, inp, d)
    off = 8 // d.y.element_size()
    n = inp.M * C
    ybuf = torch.full((off + n,), NAN, device=dev, dtype=inp.dtype)
    ybuf[off:].copy_(d.y.reshape(-1))
    zbuf = torch.full((off + n + 64,), NAN, device=dev, dtype=inp.dtype)
    yv, zv = ybuf[off:], zbuf[off:off + n]
    assert yv.data_ptr() % 16 == 8 and zv.data_ptr() % 16 == 8
    _bn_fwd(dev, inp, d, y=yv, z=zv)
    torch.cuda.synchronize()
    assert _untouched(guard, zbuf[:off], zbuf[off + n:]), "a store outside the output"
    assert torch.equal(zv.view(inp.M, C), z), "the element-wise and the 8-wide form differ"


# ---- BatchNorm + Swish backward -------------------------------------------------------------------------------------------------------
def _bn_bwd(dev, inp, d, dgamma, dbeta, sums_only=False):
    """-> dy (None for the sums alone), the two means read from the scratch, guards"""
    from emoasr_amd import lib
    M, C = inp.M, inp.C
    dy, g0 = _nan_out(dev, (M, C), inp.dtype)
    n = lib.size_query("emoasr_bn_swish_bwd_scratch_floats", M, C)
    scratch, g1 = _nan_out(dev, (n,), F32)
    if sums_only:
        tot = ctypes.c_void_p()
        lib.call("emoasr_bn_swish_bwd_sums", _code(inp.dtype), M, C, _p(d.dz), _p(d.y), _p(d.mean), _p(d.var), _p(d.gamma), _p(d.beta),
                 inp.eps, _p(dgamma), _p(dbeta), _p(scratch), ctypes.byref(tot), _stream())
        assert tot.value == scratch.data_ptr() + (n - 2 * C) * 4
        return None, scratch[n - 2 * C:], (g1,)
    lib.call("emoasr_bn_swish_bwd", _code(inp.dtype), M, C, _p(d.dz), _p(d.y), _p(d.mean), _p(d.var), _p(d.gamma), _p(d.beta),
             inp.eps, _p(dy), _p(dgamma), _p(dbeta), _p(scratch), _stream())
    return dy, scratch[n - 2 * C:], (g0, g1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.BN_BWD_CASES, ids=R.case_id)
def test_bn_swish_bwd(dev, case, dtype):
    inp = R.bn_inputs(case, R.dtype_of(dtype))
    d = _bn_dev(dev, inp)
    dg, db, ga = _acc_bufs(dev, inp)
    dy, tot, guards = _bn_bwd(dev, inp, d, dg, db)
    torch.cuda.synchronize()
    assert _untouched(*guards, *ga), "a store behind an output"
    C = inp.C
    _report(f"bn_swish_bwd {case[3]}", dtype, case, R.check_bn_bwd(inp, _cpu(dy), _cpu(dg), _cpu(db), _cpu(tot[:C]), _cpu(tot[C:])))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [("bwd", 7, 264, "randn"), ("bwd", 65, 520, "randn"), ("bwd", 4097, 8, "randn")], ids=R.case_id)
def test_bn_swish_bwd_sums_alone(dev, case, dtype):
    """emoasr_bn_swish_bwd_sums: its `tot` is the means the reference computes, dgamma / dbeta accumulate; with neither asked for
    the means are the same bit for bit"""
    assert case in R.BN_BWD_CASES
    inp = R.bn_inputs(case, R.dtype_of(dtype))
    d = _bn_dev(dev, inp)
    dg, db, ga = _acc_bufs(dev, inp)
    _, tot, guards = _bn_bwd(dev, inp, d, dg, db, sums_only=True)
    _, tot0, guards0 = _bn_bwd(dev, inp, d, None, None, sums_only=True)
    torch.cuda.synchronize()
    assert _untouched(*guards, *guards0, *ga), "a store behind an output"
    assert torch.equal(tot, tot0)
    C = inp.C
    _report("bn_swish_bwd sums", dtype, case, R.check_bn_bwd(inp, None, _cpu(dg), _cpu(db), _cpu(tot[:C]), _cpu(tot[C:])))


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_swish_bwd_refuses_c_not_a_multiple_of_8(dev, dtype):
    from emoasr_amd import lib
    inp = R.bn_inputs(("fwd", 17, 12, "randn"), R.dtype_of(dtype))
    d = _bn_dev(dev, inp)
    dg, db, ga = _acc_bufs(dev, inp)
    dy, g0 = _nan_out(dev, (inp.M, inp.C), inp.dtype)
    scratch = torch.empty(lib.size_query("emoasr_bn_swish_bwd_scratch_floats", inp.M, inp.C), device=dev, dtype=F32)
    with pytest.raises(lib.EmoasrHipError, match="multiple of 8"):
        lib.call("emoasr_bn_swish_bwd", _code(inp.dtype), inp.M, inp.C, _p(d.dz), _p(d.y), _p(d.mean), _p(d.var), _p(d.gamma),
                 _p(d.beta), inp.eps, _p(dy), _p(dg), _p(db), _p(scratch), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dy).all()) and _untouched(g0, *ga)
    assert torch.equal(dg.cpu(), inp.dg0) and torch.equal(db.cpu(), inp.db0)


# ---- the convolution's fused statistics and their merge ----------------------------------------------------------------------------------
def _conv_stats(dev, inp, finalize_c=None):
    """emoasr_dwconv_fwd_stats + emoasr_bn_stats_finalize -> y, mean, var, running mean, running var, num_batches_tracked, guards"""
    from emoasr_amd import lib
    _, B, T, C, K = inp.case
    x, w, bias = _up(dev, inp.x, inp.dtype), _up(dev, inp.w), _up(dev, inp.bias)
    y, g0 = _nan_out(dev, (B, T, C), inp.dtype)
    part = torch.full((lib.size_query("emoasr_dwconv_stats_floats", B, T, C),), NAN, device=dev, dtype=F32)
    lib.call("emoasr_dwconv_fwd_stats", _code(inp.dtype), B, T, C, K, _p(x), _p(w), _p(bias), _p(y), _p(part), _stream())
    (mean, g1), (var, g2), (rm, g3), (rv, g4) = (_nan_out(dev, (C,), F32) for _ in range(4))
    rm.copy_(inp.rm0)
    rv.copy_(inp.rv0)
    nbt = torch.tensor([7, -1], device=dev, dtype=torch.int64)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(part).all()), "a partial the merge reads was not written"
    lib.call("emoasr_bn_stats_finalize", B, T, C if finalize_c is None else finalize_c, _p(part), _p(mean), _p(var), _p(rm), _p(rv),
             inp.momentum, _p(nbt), _stream())
    return y, mean, var, rm, rv, nbt, (g0, g1, g2, g3, g4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.BN_CONV_CASES, ids=R.case_id)
def test_dwconv_stats_and_finalize(dev, case, dtype):
    """the merged statistics against the reference's statistics of the convolution output the kernel itself wrote"""
    inp = R.conv_inputs(case, R.dtype_of(dtype))
    y, mean, var, rm, rv, nbt, guards = _conv_stats(dev, inp)
    torch.cuda.synchronize()
    assert _untouched(*guards), "a store behind an output"
    assert nbt.tolist() == [8, -1], "num_batches_tracked advances by one"
    assert bool(torch.isfinite(y).all())
    res = R.check_bn_stats(inp, _cpu(mean), _cpu(var), _cpu(rm), _cpu(rv), y=_cpu(y).reshape(-1, case[3]))
    _report("bn_stats_finalize", dtype, case, res)


def test_bn_stats_finalize_refuses_more_than_64_channel_groups(dev):
    """cdiv(C, 16) <= 64 is accepted (conv-2-33-1024-7 above), 65 groups are refused and nothing is written"""
    from emoasr_amd import lib
    inp = R.conv_inputs(("conv", 1, 5, 1040, 7), F32)
    with pytest.raises(lib.EmoasrHipError, match="too wide"):
        _conv_stats(dev, inp)
    # (the buffers of the refused call are out of reach: once more by hand)
    C = 1040
    part = torch.zeros(lib.size_query("emoasr_dwconv_stats_floats", 1, 5, C), device=dev)
    (mean, g1), (var, g2) = _nan_out(dev, (C,), F32), _nan_out(dev, (C,), F32)
    rm, rv, nbt = torch.ones(C, device=dev), torch.ones(C, device=dev), torch.tensor([7], device=dev, dtype=torch.int64)
    with pytest.raises(lib.EmoasrHipError, match="too wide"):
        lib.call("emoasr_bn_stats_finalize", 1, 5, C, _p(part), _p(mean), _p(var), _p(rm), _p(rv), 0.1, _p(nbt), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(mean).all()) and bool(torch.isnan(var).all()) and _untouched(g1, g2)
    assert bool((rm == 1).all()) and bool((rv == 1).all()) and int(nbt) == 7
