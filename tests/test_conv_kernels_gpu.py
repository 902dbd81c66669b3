"""The GLU kernels of csrc/elementwise.hip, the depthwise-convolution kernels of csrc/convmodule.hip and the fused convolution-module
kernels of csrc/convfused.hip against the float64 restatement of tests/conv_ref.py (pinned on the CPU by
tests/test_conv_ref_cpu.py), through the C ABI with the test's own buffers: every output is NaN-filled with a 64-element NaN guard
behind it (after the launch every defined element is finite, the guard untouched), the weight-gradient scratch is NaN-filled, dw / db
start from non-zero random values (the expectation is start + reference), options are set by lib.options scopes only.  Bounds:
tests/norm_ref.py through tests/conv_ref.py (element outputs, the order-independent column-sum bound; none taken from the kernels).

PATH COVERAGE, from the dispatch conditions (ids of conv_ref's tables):
  emoasr_dwconv_fwd / _fwd_stats / _bwd_x: use_lds = option dwconv_lds && bf16 && C % 8 == 0 -> cf_dwconv_kernel<false> (strips of
  S tiles, S = option conv_strip, 0 = the rule below); otherwise dwconv_kernel<T>
    dwconv_kernel<float>        every id of DW_CASES (taps-*, time-*, chan-*, batch-*) and options-* as "f32"
    dwconv_kernel<bf16>         the same as "bf16-plain" (dwconv_lds = 0), strips-* too; under dwconv_lds = 1 the ids with C % 8 != 0:
                                chan-2-33-{1,12,260,300}-15, options-2-33-12-31 ("bf16-fallback")
    cf_dwconv_kernel<false>     "bf16-lds": taps-*, time-*, chan-2-33-{8..520}-15, batch-*, options-2-70-264-15 and strips-* at every
                                S of (1, 2, 3, 4, 8, 0) (one-tile utterances: S = 1 and 0); flip = 1 through emoasr_dwconv_bwd_x, the
                                statistics table through emoasr_dwconv_fwd_stats
  emoasr_dwconv_bwd_w: dwconv_bwd_w_kernel<T> + the reduce in ONE slice, always
    <float>, <bf16>             every id of DW_CASES, strips-*, reduce-* (1023 and 1024 partial rows), options-*
  emoasr_glu_dwconv_fwd (bf16, C % 8 == 0; everything else is refused) -> cf_dwconv_kernel<true>
                                test_chain_is_bit_identical_over_the_edge_tables (training: with the statistics table; eval: without),
                                test_exact_tap_counts, test_strip_rule: every id of CHAIN_CASES x every S
  emoasr_conv_bwd_fused (bf16, C % 8 == 0) -> cf_conv_bwd_kernel with per_tile = 1, then emo_dwconv_bwd_w_reduce
                                the same tests, every S; S chosen by the rule: test_strip_rule (rule-*: S = 2 and S = 8 on the
                                device's CU count); per_tile = 0 is the stacked entry's (tests/test_conv_strip_gpu.py)
  the rule (strip_tiles, conv_strip = 0): the smallest S <= 8 with B cdiv(cdiv(T, 32), S) cdiv(C, 256) <= 2 CUs
  emo_dwconv_bwd_w_reduce: gridDim.y = nblk >= 1024 ? 4 : 1, nblk = B cdiv(T, 32); four slices meet in float atomics
    one slice                   every conv_bwd_fused call above but the two below; reduce-33-992-8-{7,31} (1023 rows)
    four slices                 reduce-32-1024-8-{7,31} (1024 rows), rule-*-512-8-7 (2736 rows on 256 CUs), and the ones-filled
                                reduce shapes of test_exact_tap_counts
  emoasr_glu_fwd / _bwd / _fwd_masked: one grid-stride kernel each per dtype: glu-*, glum-*

MEASURED on an MI355X, worst share of the bound per family (the `[measured] conv <family>` lines this module prints when it is
done; f32 | bf16 on the plain kernel | bf16 on the LDS kernel, the worst over its strip lengths).  Wall time of the module's 722
tests: 6 - 8 s.
  glu_fwd       randn out 0.087 | 0.995          hard out 0.155 | 0.976          masked out 0.076 | 0.980
  glu_bwd       randn din 0.205 | 0.994          hard din 0.250 | 0.976
  dwconv_fwd    taps  y 0.250 | 0.988 | 0.988    time y 0.317 | 0.988 | 0.988    chan y 0.247 | 0.995 | 0.994 (C % 8 != 0: 0.995)
                batch y 0.250 | 0.983 | 0.983    strips y - | 0.995 | 0.995      bias = None y 0.185 | 0.993 | 0.993
  dwconv_bwd_x  taps  dx 0.219 | 0.995 | 0.995   time dx 0.227 | 0.988 | 0.988   chan dx 0.258 | 0.995 | 0.995
                batch dx 0.250 | 0.981 | 0.981   strips dx - | 0.995 | 0.995
  dwconv_bwd_w  taps  dw 0.008, db 0.004 | dw 0.005, db 0.002      time  dw 0.072, db 0.060 | dw 0.045, db 0.036
                chan  dw 0.035, db 0.031 | dw 0.023, db 0.005      batch dw 0.069, db 0.067 | dw 0.074, db 0.017
                strips dw 0.003, db 0.003 | dw 0.003, db 0.001     reduce (1023 / 1024 rows) all 0.000 (below 5e-4)
                accumulate = 1 dw 0.016, db 0.010 | dw 0.010, db 0.002      accumulate = 0 the same to 0.001
  strip rule    S = 2 (52 x 289 frames on 256 CUs): gl 0.993, y 0.994, dx 0.994, dg 0.994, dw / db 0.000
                S = 8 (171 x 512 frames, 2736 tiles): gl 0.996, y 0.995, dx 0.995, dg 0.995, dw / db 0.000; the fused entry's
                four-slice dw / db 0.000
  fold          1023 tiles (33 x 992, K = 7 and 31): two fused calls equal, fused equals unfused; dw / db 0.000 of the bound
                1024 tiles (32 x 1024, K = 7 and 31): two fused calls NOT equal, fused NOT equal to unfused; dw / db 0.000
Every share near 1 is a bf16 ELEMENT output: the term of its bound that is reached is 2^-8 |ref|, bf16's worst rounding, which is
the bound by construction; the f32 column beside it shows the arithmetic before that rounding at a third of its bound or less
(0.250 = a bound of 4 e32 with the kernel one rounding from the model).  The column sums use a
fourteenth of their bounds at most; over the 32 768 rows of the reduce shapes R 2^-24 sum |term| is wide (the shares print as
0.000), yet a missing slice still leaves it (planted error 3 below), and the ones-filled shapes of test_exact_tap_counts see it
exactly.

What the sweep exposed: no wrong result -- every kernel on every path above held every bound, every closed form, every
bit-identity below 1024 tiles (T = 1 and T <= pad included), every NaN guard and every refusal -- and ONE false promise: the header
of csrc/convfused.hip, include/emoasr_hip.h, DESIGN.md and tests/test_conv_strip_gpu.py said that emoasr_conv_bwd_fused gives the
unfused kernels' dw / dbias bit for bit.  At B cdiv(T, 32) >= 1024 it does not (the lines above), and its dw / dbias then differ
from call to call.  Both sides are inside the f64 bound; the four-slice fold is kept (its speed is not measured here) and the four
texts now say "below 1024 tiles".

That the module can fail was tried on a scratch build with three errors planted, each a wrong answer inside every buffer:
  (1) the forward tap offset taken as 15 where (K - 1) / 2 is meant, in dwconv_kernel AND in the staging of cf_dwconv_kernel (the
      ring's geometry left alone): the present suite (tests/test_conv_strip_gpu.py, the convolution tests of tests/test_ops_gpu.py
      and tests/test_norm_kernels_gpu.py: 103 tests) passes -- its only reference runs K = 31, and every K < 31 shape compares
      two kernels that are wrong alike.  Here 140 tests fail: test_dwconv_fwd (101: every K < 31 id on every path),
      test_exact_tap_counts (35), test_dwconv_options (3), test_strip_rule[S=8] (K = 7); the chain test passes, as it must.
  (2) a strip's restaged rows start at t0 + 30 instead of t0 + 2 pad (both strip kernels): the present suite sees this one
      (8 cases of test_conv_strip_gpu.py, dense and stacked: K < 31 at S >= 2).  Here 81 fail: test_dwconv_fwd and
      test_dwconv_bwd_x (19 each: the K < 31 ids of more than one tile on the LDS path), the chain (19),
      test_exact_tap_counts (21), test_strip_rule[S=8] (K = 7), test_weight_gradient_fold_at_1024_tiles (2: K = 7, dg).
  (3) the four-slice reduce drops its last slice: the present suite passes (no dense test reaches 1024 tiles).  Here 5 fail:
      test_exact_tap_counts (the two ones-filled 1024-tile shapes), test_weight_gradient_fold_at_1024_tiles (2),
      test_strip_rule[S=8] (2736 tiles)."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from tests import conv_ref as R

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
# path -> (dtype, the dwconv_lds option)
PATHS = {"f32": (F32, 1), "bf16-plain": (BF, 0), "bf16-lds": (BF, 1), "bf16-fallback": (BF, 1)}


def _nan_out(dev, shape, dtype):
    """a NaN-filled tensor of this shape with 64 NaN guard elements behind it -> (tensor, guard)"""
    n = 1
    for v in shape:
        n *= v
    flat = torch.full((n + 64,), NAN, device=dev, dtype=dtype)
    return flat[:n].view(*shape), flat[n:]


def _start_out(dev, start):
    """a float32 accumulator holding its start value, with a NaN guard behind it"""
    t, g = _nan_out(dev, tuple(start.shape), F32)
    t.copy_(start)
    return t, g


def _untouched(guards):
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


def _up(dev, t, dtype=F32):
    return None if t is None else t.to(dtype).to(dev).contiguous()


_WORST = {}      # family -> path -> tensor -> worst share of the bound over the family's cases


def _report(family, path, case, res):
    """every case must be inside its bounds; the worst shares are kept per family and path and printed once, when the module is done"""
    w = _WORST.setdefault(family, {}).setdefault(path, {})
    for k, v in res.items():
        w[k] = max(v, w.get(k, 0.0))
    assert max(res.values()) <= 1.0, (family, path, case, res)


_NOTES = []


@pytest.fixture(scope="module", autouse=True)
def _measured():
    yield
    for family, by_path in _WORST.items():
        print(f"\n[measured] conv {family}: " + " | ".join(p + " " + ", ".join(f"{k} {v:.3f}" for k, v in w.items())
                                                            for p, w in by_path.items()), end="")
    for note in _NOTES:
        print(f"\n[measured] conv {note}", end="")
    print()


_INPUTS = {}


def _inputs(case, dtype):
    """one input set per (case, dtype) for the whole module: its reference and model evaluations are computed once and never modified"""
    if (case, dtype) not in _INPUTS:
        _INPUTS[(case, dtype)] = R.glu_inputs(case, dtype) if case[0].startswith("glu") else R.conv_inputs(case, dtype)
    return _INPUTS[(case, dtype)]


def _tiles(case):
    return R.cdiv(case[2], 32)


def _s_list(case, path="bf16-lds"):
    """the strip lengths that differ for this case on a strip kernel; the other kernels ignore the option"""
    if path != "bf16-lds":
        return (0,)
    return R.STRIP_S if _tiles(case) > 1 else (1, 0)


# ---- launches on the test's own buffers ---------------------------------------------------------------------------------------------
def _glu(dev, op, g, d=None, lens=None):
    """g [M, 2C] (masked: [B, T, 2C]) -> out, guard"""
    from emoasr_amd import lib
    C = g.shape[-1] // 2
    M = g.numel() // (2 * C)
    if op == "fwd":
        out, gd = _nan_out(dev, (M, C), g.dtype)
        lib.call("emoasr_glu_fwd", _code(g.dtype), M, C, _p(g), _p(out), _stream())
    elif op == "masked":
        out, gd = _nan_out(dev, tuple(g.shape[:2]) + (C,), g.dtype)
        lib.call("emoasr_glu_fwd_masked", _code(g.dtype), g.shape[0], g.shape[1], C, _p(g), _p(lens), _p(out), _stream())
    else:
        out, gd = _nan_out(dev, (M, 2 * C), g.dtype)
        lib.call("emoasr_glu_bwd", _code(g.dtype), M, C, _p(g), _p(d), _p(out), _stream())
    return out, gd


def _dw_fwd(dev, x, w, bias, K, stats=False, guards=None):
    """-> y (and the statistics table, NaN-filled before the call)"""
    from emoasr_amd import lib
    B, T, C = x.shape
    y, g0 = _nan_out(dev, (B, T, C), x.dtype)
    guards.append(g0)
    if not stats:
        lib.call("emoasr_dwconv_fwd", _code(x.dtype), B, T, C, K, _p(x), _p(w), _p(bias), _p(y), _stream())
        return y
    part, g1 = _nan_out(dev, (lib.size_query("emoasr_dwconv_stats_floats", B, T, C),), F32)
    guards.append(g1)
    lib.call("emoasr_dwconv_fwd_stats", _code(x.dtype), B, T, C, K, _p(x), _p(w), _p(bias), _p(y), _p(part), _stream())
    return y, part


def _dw_bwd_x(dev, dy, w, K, guards):
    from emoasr_amd import lib
    B, T, C = dy.shape
    dx, g0 = _nan_out(dev, (B, T, C), dy.dtype)
    guards.append(g0)
    lib.call("emoasr_dwconv_bwd_x", _code(dy.dtype), B, T, C, K, _p(dy), _p(w), _p(dx), _stream())
    return dx


def _dw_bwd_w(dev, dy, x, K, dw, db, accumulate, guards):
    from emoasr_amd import lib
    B, T, C = dy.shape
    scratch, g0 = _nan_out(dev, (lib.size_query("emoasr_dwconv_bwd_w_scratch_floats", B, T, C, K),), F32)
    guards.append(g0)
    lib.call("emoasr_dwconv_bwd_w", _code(dy.dtype), B, T, C, K, _p(dy), _p(x), _p(dw), _p(db), int(accumulate), _p(scratch), _stream())


def _finalize(dev, B, T, C, part, guards):
    from emoasr_amd import lib
    (mean, g0), (var, g1) = _nan_out(dev, (C,), F32), _nan_out(dev, (C,), F32)
    guards += [g0, g1]
    lib.call("emoasr_bn_stats_finalize", B, T, C, _p(part), _p(mean), _p(var), None, None, 0.1, None, _stream())
    return mean, var


def _fused_fwd(dev, g, B, T, C, K, w, bias, stats, guards, dtype=None):
    """emoasr_glu_dwconv_fwd on g [B*T, 2C] -> c [B, T, C] (and the statistics table)"""
    from emoasr_amd import lib
    c, g0 = _nan_out(dev, (B, T, C), g.dtype)
    guards.append(g0)
    part = None
    if stats:
        part, g1 = _nan_out(dev, (lib.size_query("emoasr_dwconv_stats_floats", B, T, C),), F32)
        guards.append(g1)
    lib.call("emoasr_glu_dwconv_fwd", _code(dtype or g.dtype), B, T, C, K, _p(g), _p(w), _p(bias), _p(c), _p(part), _stream())
    return (c, part) if stats else c


def _fused_bwd(dev, B, T, C, K, ds, cv, mean, var, gamma, beta, tot, g, w, dw, db, guards, dtype=None):
    """emoasr_conv_bwd_fused -> dg [B*T, 2C]; dw / db are accumulated into; tot: the [2][C] BatchNorm means"""
    from emoasr_amd import lib
    dg, g0 = _nan_out(dev, (B * T, 2 * C), g.dtype)
    scratch, g1 = _nan_out(dev, (lib.size_query("emoasr_dwconv_bwd_w_scratch_floats", B, T, C, max(K, 0)),), F32)
    guards += [g0, g1]
    lib.call("emoasr_conv_bwd_fused", _code(dtype or g.dtype), B, T, C, K, _p(ds), _p(cv), _p(mean), _p(var), _p(gamma), _p(beta),
             R.EPS, tot if isinstance(tot, ctypes.c_void_p) else _p(tot), _p(g), _p(w), _p(dg), _p(dw), _p(db), _p(scratch), _stream())
    return dg


def _bn_bwd(dev, M, C, ds, c, mean, var, gamma, beta, dgam, dbet, sums_only, keep, guards):
    """emoasr_bn_swish_bwd -> dc, or emoasr_bn_swish_bwd_sums -> the device pointer of the [2][C] means inside the scratch (kept
    alive in `keep`)"""
    from emoasr_amd import lib
    scratch = torch.empty(lib.size_query("emoasr_bn_swish_bwd_scratch_floats", M, C), device=dev, dtype=F32)
    keep.append(scratch)
    if sums_only:
        tot = ctypes.c_void_p()
        lib.call("emoasr_bn_swish_bwd_sums", _code(BF), M, C, _p(ds), _p(c), _p(mean), _p(var), _p(gamma), _p(beta), R.EPS, _p(dgam),
                 _p(dbet), _p(scratch), ctypes.byref(tot), _stream())
        return tot
    dc, g0 = _nan_out(dev, (M, C), BF)
    guards.append(g0)
    lib.call("emoasr_bn_swish_bwd", _code(BF), M, C, _p(ds), _p(c), _p(mean), _p(var), _p(gamma), _p(beta), R.EPS, _p(dc), _p(dgam),
             _p(dbet), _p(scratch), _stream())
    return dc


def _dev_inputs(dev, inp):
    dt, M = inp.dtype, inp.B * inp.T
    return SimpleNamespace(x=_up(dev, inp.x, dt), dy=_up(dev, inp.dy, dt), g=_up(dev, inp.g, dt).view(M, 2 * inp.C),
                           ds=_up(dev, inp.ds, dt).view(M, inp.C), w=_up(dev, inp.w), bias=_up(dev, inp.bias),
                           gamma=_up(dev, inp.gamma), beta=_up(dev, inp.beta))


# ---- GLU ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.GLU_CASES, ids=R.case_id)
def test_glu_fwd(dev, case, dtype):
    inp = _inputs(case, R.F32 if dtype == "f32" else BF)
    out, guard = _glu(dev, "fwd", _up(dev, inp.g, inp.dtype))
    torch.cuda.synchronize()
    assert _untouched([guard]), "a store behind the output"
    _report(f"glu_fwd {case[3]}", dtype, case, R.check_glu(inp, "fwd", _cpu(out)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.GLU_CASES, ids=R.case_id)
def test_glu_bwd(dev, case, dtype):
    inp = _inputs(case, R.F32 if dtype == "f32" else BF)
    din, guard = _glu(dev, "bwd", _up(dev, inp.g, inp.dtype), d=_up(dev, inp.d, inp.dtype))
    torch.cuda.synchronize()
    assert _untouched([guard]), "a store behind the output"
    _report(f"glu_bwd {case[3]}", dtype, case, R.check_glu(inp, "bwd", _cpu(din)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.GLU_MASKED_CASES, ids=R.case_id)
def test_glu_fwd_masked(dev, case, dtype):
    """zeros at t >= lens[b] are exact zeros; the live frames are emoasr_glu_fwd's bit for bit"""
    inp = _inputs(case, R.F32 if dtype == "f32" else BF)
    g = _up(dev, inp.g, inp.dtype)
    out, guard = _glu(dev, "masked", g, lens=inp.lens.to(dev))
    plain, guard1 = _glu(dev, "fwd", g)
    torch.cuda.synchronize()
    assert _untouched([guard, guard1]), "a store behind the output"
    _report("glu_fwd_masked", dtype, case, R.check_glu(inp, "masked", _cpu(out)))
    plain = plain.view_as(out)
    for b, n in enumerate(case[4]):
        assert bool((out[b, n:] == 0).all()) and torch.equal(out[b, :n], plain[b, :n])


# ---- the depthwise convolution against f64 --------------------------------------------------------------------------------------------
def _paths_of(case):
    if case[0] == "strips":
        return ("bf16-plain", "bf16-lds")
    return ("f32", "bf16-plain", "bf16-lds") if case[3] % 8 == 0 else ("f32", "bf16-plain", "bf16-fallback")


_DW_PARAMS = [pytest.param(case, path, id=f"{R.case_id(case)}-{path}") for case in R.DW_CASES + R.STRIPS for path in _paths_of(case)]


@pytest.mark.parametrize("case,path", _DW_PARAMS)
def test_dwconv_fwd(dev, case, path):
    """at every strip length of the path; the y of emoasr_dwconv_fwd_stats is the y of emoasr_dwconv_fwd bit for bit and its table
    is written in full"""
    from emoasr_amd import lib
    dtype, lds = PATHS[path]
    inp = _inputs(case, dtype)
    d = _dev_inputs(dev, inp)
    for S in _s_list(case, path):
        guards = []
        with lib.options(dwconv_lds=lds, conv_strip=S):
            y = _dw_fwd(dev, d.x, d.w, d.bias, inp.K, guards=guards)
            ys, part = _dw_fwd(dev, d.x, d.w, d.bias, inp.K, stats=True, guards=guards)
        torch.cuda.synchronize()
        assert _untouched(guards), "a store behind an output"
        assert torch.equal(ys, y), f"S={S}: y depends on whether the statistics are asked for"
        assert bool(torch.isfinite(part).all()), f"S={S}: a statistics partial was not written"
        _report(f"dwconv_fwd {case[0]}", path, (case, S), R.check_fwd(inp, _cpu(y)))


@pytest.mark.parametrize("case,path", _DW_PARAMS)
def test_dwconv_bwd_x(dev, case, path):
    from emoasr_amd import lib
    dtype, lds = PATHS[path]
    inp = _inputs(case, dtype)
    d = _dev_inputs(dev, inp)
    for S in _s_list(case, path):
        guards = []
        with lib.options(dwconv_lds=lds, conv_strip=S):
            dx = _dw_bwd_x(dev, d.dy, d.w, inp.K, guards)
        torch.cuda.synchronize()
        assert _untouched(guards), "a store behind an output"
        _report(f"dwconv_bwd_x {case[0]}", path, (case, S), R.check_bwd_x(inp, _cpu(dx)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.DW_CASES + R.STRIPS + R.REDUCE, ids=R.case_id)
def test_dwconv_bwd_w(dev, case, dtype):
    """accumulate = 1 onto non-zero random dw / db: start + reference (one kernel per dtype, no LDS form; the fold is one slice)"""
    inp = _inputs(case, R.F32 if dtype == "f32" else BF)
    d = _dev_inputs(dev, inp)
    guards = []
    (dw, g0), (db, g1) = _start_out(dev, inp.dw0), _start_out(dev, inp.db0)
    _dw_bwd_w(dev, d.dy, d.x, inp.K, dw, db, 1, guards)
    torch.cuda.synchronize()
    assert _untouched(guards + [g0, g1]), "a store behind an output"
    _report(f"dwconv_bwd_w {case[0]}", dtype, case, R.check_bwd_w(inp, _cpu(dw), _cpu(db)))


@pytest.mark.parametrize("case,path", [pytest.param(case, path, id=f"{R.case_id(case)}-{path}") for case in R.OPTIONS
                                       for path in _paths_of(case)])
def test_dwconv_options(dev, case, path):
    """bias = None (forward, with and without the statistics); dbias = None (db is not needed and dw is the same bit for bit);
    accumulate = 0 onto NaN-filled dw / db stores the sums; accumulate = 1 is start + sum"""
    from emoasr_amd import lib
    dtype, lds = PATHS[path]
    inp = _inputs(case, dtype)
    d = _dev_inputs(dev, inp)
    guards = []
    with lib.options(dwconv_lds=lds):
        y = _dw_fwd(dev, d.x, d.w, None, inp.K, guards=guards)
        ys, _ = _dw_fwd(dev, d.x, d.w, None, inp.K, stats=True, guards=guards)
        (dw, g0), (db, g1) = _start_out(dev, inp.dw0), _start_out(dev, inp.db0)
        _dw_bwd_w(dev, d.dy, d.x, inp.K, dw, db, 1, guards)
        dw1, g2 = _start_out(dev, inp.dw0)
        _dw_bwd_w(dev, d.dy, d.x, inp.K, dw1, None, 1, guards)
        (dwn, g3), (dbn, g4) = _nan_out(dev, (inp.C, inp.K), F32), _nan_out(dev, (inp.C,), F32)
        _dw_bwd_w(dev, d.dy, d.x, inp.K, dwn, dbn, 0, guards)
        dwn1, g5 = _nan_out(dev, (inp.C, inp.K), F32)
        _dw_bwd_w(dev, d.dy, d.x, inp.K, dwn1, None, 0, guards)
    torch.cuda.synchronize()
    assert _untouched(guards + [g0, g1, g2, g3, g4, g5]), "a store behind an output"
    assert torch.equal(ys, y)
    _report("options bias=None", path, case, R.check_fwd(inp, _cpu(y), bias=False))
    _report("options accumulate=1", path, case, R.check_bwd_w(inp, _cpu(dw), _cpu(db)))
    _report("options accumulate=0", path, case, R.check_bwd_w(inp, _cpu(dwn), _cpu(dbn), accumulate=False))
    assert torch.equal(dw1, dw) and torch.equal(dwn1, dwn), "dw depends on whether dbias is asked for"


# ---- the exact cases ------------------------------------------------------------------------------------------------------------------
def _exact_shapes():
    seen = []
    for case in R.CHAIN_CASES + R.REDUCE:
        s = (case[1], case[2], case[3], case[4])
        if s not in seen:
            seen.append(s)
    return seen


@pytest.mark.parametrize("shape", _exact_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_exact_tap_counts(dev, shape):
    """x = 1, w = 1, no bias: y[t] = dx[t] = the taps inside the utterance; dy = 1, x = 1: dw[c, j] = B max(0, T - |j - pad|),
    db = B T -- integers that every float32 order gives exactly, so torch.equal on every path and every S: both plain kernels, the
    LDS kernel, and the fused kernels.  There the GLU input is a = 1 with the gate at 90 (sigmoid = 1 in float32, so z = 1 and the
    gate gradient dz a s (1 - s) is 0), and dc = 1 is built as in tests/test_conv_strip_gpu.py: c = 1, mean 0, var 1 - eps,
    gamma -1, beta 1, ds = 2 and both BatchNorm means 1 give xhat = 1, dbn = 2 swish'(0) = 1, dc = -1 (1 - 1 - 1) = 1 after the
    rounding to bf16."""
    from emoasr_amd import lib
    B, T, C, K = shape
    case = ("exact",) + shape
    counts = R.tap_counts(T, K).to(dev)[None, :, None].expand(B, T, C)
    dwc = R.dw_counts(B, T, K).to(dev)[None, :].expand(C, K)
    w = torch.ones(C, K, device=dev)
    guards = []

    def zeros():
        (dw, g0), (db, g1) = _start_out(dev, torch.zeros(C, K)), _start_out(dev, torch.zeros(C))
        guards.extend([g0, g1])
        return dw, db

    for path in ("f32", "bf16-plain", "bf16-lds"):
        dtype, lds = PATHS[path]
        one = torch.ones(B, T, C, device=dev, dtype=dtype)
        for S in _s_list(case, path):
            with lib.options(dwconv_lds=lds, conv_strip=S):
                y = _dw_fwd(dev, one, w, None, K, guards=guards)
                dx = _dw_bwd_x(dev, one, w, K, guards)
            assert torch.equal(y.float(), counts), f"{path} S={S}: y"
            assert torch.equal(dx.float(), counts), f"{path} S={S}: dx"
        dw, db = zeros()
        _dw_bwd_w(dev, one, one, K, dw, db, 1, guards)
        assert torch.equal(dw, dwc) and torch.equal(db, torch.full_like(db, float(B * T))), f"{path}: dw / db"
    # the fused kernels
    M = B * T
    g = torch.cat([torch.ones(M, C), torch.full((M, C), 90.0)], 1).to(dev, BF)
    ds, cv = torch.full((M, C), 2.0, device=dev, dtype=BF), torch.ones(M, C, device=dev, dtype=BF)
    mean, var = torch.zeros(C, device=dev), torch.full((C,), 1 - R.EPS, device=dev)
    gamma, beta, tot = -torch.ones(C, device=dev), torch.ones(C, device=dev), torch.ones(2, C, device=dev)
    for S in _s_list(case):
        with lib.options(conv_strip=S):
            c = _fused_fwd(dev, g, B, T, C, K, w, None, False, guards)
            dw, db = zeros()
            dg = _fused_bwd(dev, B, T, C, K, ds, cv, mean, var, gamma, beta, tot, g, w, dw, db, guards)
        assert torch.equal(c.float(), counts), f"fused S={S}: c"
        assert torch.equal(dg[:, :C].float().view(B, T, C), counts) and bool((dg[:, C:] == 0).all()), f"fused S={S}: dg"
        assert torch.equal(dw, dwc) and torch.equal(db, torch.full_like(db, float(B * T))), f"fused S={S}: dw / db"
    torch.cuda.synchronize()
    assert _untouched(guards), "a store behind an output"


# ---- the chain of bit-identities ------------------------------------------------------------------------------------------------------
def _chain_unfused(dev, d, B, T, C, K, guards, keep):
    """GLU -> depthwise convolution (training: with statistics; eval) -> [BatchNorm / Swish backward] -> data gradient, weight
    gradient -> GLU backward, one launch each"""
    M = B * T
    gl, g0 = _glu(dev, "fwd", d.g)
    guards.append(g0)
    gl3 = gl.view(B, T, C)
    c, part = _dw_fwd(dev, gl3, d.w, d.bias, K, stats=True, guards=guards)
    mean, var = _finalize(dev, B, T, C, part, guards)
    c_eval = _dw_fwd(dev, gl3, d.w, d.bias, K, guards=guards)
    dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    dc = _bn_bwd(dev, M, C, d.ds, c.view(M, C), mean, var, d.gamma, d.beta, dgam, dbet, False, keep, guards)
    dgl = _dw_bwd_x(dev, dc.view(B, T, C), d.w, K, guards)
    (dw, g1), (db, g2) = _start_out(dev, torch.zeros(C, K)), _start_out(dev, torch.zeros(C))
    _dw_bwd_w(dev, dc.view(B, T, C), gl3, K, dw, db, 1, guards)
    dg, g3 = _glu(dev, "bwd", d.g, d=dgl.view(M, C))
    guards += [g1, g2, g3]
    return dict(gl=gl, c=c, mean=mean, var=var, c_eval=c_eval, dgam=dgam, dbet=dbet, dc=dc, dgl=dgl, dw=dw, db=db, dg=dg)


def _chain_fused(dev, d, B, T, C, K, guards, keep):
    M = B * T
    c, part = _fused_fwd(dev, d.g, B, T, C, K, d.w, d.bias, True, guards)
    mean, var = _finalize(dev, B, T, C, part, guards)
    c_eval = _fused_fwd(dev, d.g, B, T, C, K, d.w, d.bias, False, guards)
    dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    tot = _bn_bwd(dev, M, C, d.ds, c.view(M, C), mean, var, d.gamma, d.beta, dgam, dbet, True, keep, guards)
    (dw, g1), (db, g2) = _start_out(dev, torch.zeros(C, K)), _start_out(dev, torch.zeros(C))
    dg = _fused_bwd(dev, B, T, C, K, d.ds, c.view(M, C), mean, var, d.gamma, d.beta, tot, d.g, d.w, dw, db, guards)
    guards += [g1, g2]
    return dict(c=c, mean=mean, var=var, c_eval=c_eval, dgam=dgam, dbet=dbet, dw=dw, db=db, dg=dg)


def _same(got, ref, what, skip=()):
    for k, v in got.items():
        if k in ref and k not in skip:
            assert torch.equal(v, ref[k]), f"{what}: {k} differs (max {(v.float() - ref[k].float()).abs().max().item():.3e})"


@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=R.case_id)
def test_chain_is_bit_identical_over_the_edge_tables(dev, case):
    """bf16, over TAPS, TIME, CHANNELS, BATCH and STRIPS: the plain kernels (dwconv_lds = 0), the LDS kernel at every S, and
    emoasr_glu_dwconv_fwd (training and eval) + emoasr_conv_bwd_fused at every S give the same c, statistics, dg, dw and db bit for
    bit (every case has fewer than 1024 tiles: the fused entry's fold runs one slice).  The argument this closes: each unfused stage
    -- glu_fwd, dwconv_fwd, dwconv_bwd_x, dwconv_bwd_w, glu_bwd -- is held to f64 above on the operands handed in, at these very
    shapes; the fused kernels take no operand the unfused ones do not, so equality carries every one of those bounds to them."""
    from emoasr_amd import lib
    _, B, T, C, K, _ = case
    assert B * _tiles(case) < 1024 and C % 8 == 0
    inp = _inputs(case, BF)
    d = _dev_inputs(dev, inp)
    guards, keep = [], []
    with lib.options(dwconv_lds=0):
        ref = _chain_unfused(dev, d, B, T, C, K, guards, keep)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in ref.values()), "a defined element is not finite"
    for S in R.STRIP_S:
        with lib.options(dwconv_lds=1, conv_strip=S):
            lds = _chain_unfused(dev, d, B, T, C, K, guards, keep)
            got = _chain_fused(dev, d, B, T, C, K, guards, keep)
        _same(lds, ref, f"S={S}: LDS-staged")
        _same(got, ref, f"S={S}: fused")
    torch.cuda.synchronize()
    assert _untouched(guards), "a store behind an output"


def _check_stages(inp, u, family, path):
    """the unfused stages of a chain against f64, each on the operands the device handed it"""
    B, T, C, K = inp.B, inp.T, inp.C, inp.K
    gl, dc = _cpu(u["gl"]).view(B, T, C), _cpu(u["dc"]).view(B, T, C)
    res = {"gl": R.check_glu(SimpleNamespace(g=inp.g.reshape(B * T, 2 * C), dtype=BF), "fwd", _cpu(u["gl"]))["out"]}
    res.update(R.check_fwd(inp, _cpu(u["c_eval"]), x=gl))
    res.update(R.check_bwd_x(inp, _cpu(u["dgl"]), dy=dc))
    res.update(R.check_bwd_w(R.operands(gl, dc, K, BF), _cpu(u["dw"]), _cpu(u["db"])))
    res["dg"] = R.check_glu(SimpleNamespace(g=inp.g.reshape(B * T, 2 * C), d=_cpu(u["dgl"]).view(B * T, C), dtype=BF), "bwd",
                            _cpu(u["dg"]))["din"]
    _report(family, path, inp.case, res)


@pytest.mark.parametrize("which", [0, 1], ids=["S>=2", "S=8"])
def test_strip_rule(dev, which):
    """conv_strip = 0, the production rule (strip_tiles): the smallest S <= 8 with B cdiv(cdiv(T, 32), S) cdiv(C, 256) <= 2 CUs.
    conv_ref.rule_cases picks B from this device's CU count so that the rule returns S = 2 (T = 289) and S = 8 (T = 512) at C = 8;
    every other test shape of the suite is far below 2 CUs strips, where it returns 1.  The chain's equalities hold, the unfused
    stages are inside their f64 bounds on the operands handed in; with 1024 or more tiles the fused entry's fold runs four slices,
    and dw / db are then held to the f64 column-sum bound instead of to equality."""
    from emoasr_amd import lib
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    case = R.rule_cases(cus)[which]
    _, B, T, C, K, _ = case
    S = R.rule_S(B, T, C, cus)
    assert (S >= 2, S == 8)[which], (case, cus, S)
    inp = _inputs(case, BF)
    d = _dev_inputs(dev, inp)
    guards, keep = [], []
    with lib.options(dwconv_lds=0):
        ref = _chain_unfused(dev, d, B, T, C, K, guards, keep)
    with lib.options(dwconv_lds=1, conv_strip=0):
        lds = _chain_unfused(dev, d, B, T, C, K, guards, keep)
        got = _chain_fused(dev, d, B, T, C, K, guards, keep)
    torch.cuda.synchronize()
    assert _untouched(guards), "a store behind an output"
    one_slice = B * _tiles(case) < 1024
    _same(lds, ref, f"rule S={S}: LDS-staged")
    _same(got, ref, f"rule S={S}: fused", skip=() if one_slice else ("dw", "db"))
    _check_stages(inp, ref, "strip rule", f"S={S}")
    if not one_slice:
        gl, dc = _cpu(ref["gl"]).view(B, T, C), _cpu(ref["dc"]).view(B, T, C)
        _report("strip rule four-slice fold", f"S={S}", case, R.check_bwd_w(R.operands(gl, dc, K, BF), _cpu(got["dw"]), _cpu(got["db"])))


@pytest.mark.parametrize("case", R.REDUCE, ids=R.case_id)
def test_weight_gradient_fold_at_1024_tiles(dev, case):
    """emoasr_conv_bwd_fused folds its per-tile partials with emo_dwconv_bwd_w_reduce: below 1024 tiles in one slice -- the
    unfused kernel's order, dw / db bit-identical to emoasr_dwconv_bwd_w (1023 tiles: B = 33, T = 992); from 1024 tiles on in four
    slices that meet in float atomics (B = 32, T = 1024), where dw / db are held to the f64 column-sum bound on the dc and the GLU
    output the unfused kernels produced, and two calls are compared and the outcome reported, not asserted.  (The four-slice fold is
    kept: its speed is not measured here.)"""
    _, B, T, C, K, _ = case
    tiles = B * _tiles(case)
    inp = _inputs(case, BF)
    d = _dev_inputs(dev, inp)
    guards, keep = [], []
    u = _chain_unfused(dev, d, B, T, C, K, guards, keep)
    M = B * T
    runs = []
    for _ in range(2):
        dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        tot = _bn_bwd(dev, M, C, d.ds, u["c"].view(M, C), u["mean"], u["var"], d.gamma, d.beta, dgam, dbet, True, keep, guards)
        (dw, g1), (db, g2) = _start_out(dev, torch.zeros(C, K)), _start_out(dev, torch.zeros(C))
        dg = _fused_bwd(dev, B, T, C, K, d.ds, u["c"].view(M, C), u["mean"], u["var"], d.gamma, d.beta, tot, d.g, d.w, dw, db, guards)
        guards += [g1, g2]
        runs.append((dg, dw, db))
    torch.cuda.synchronize()
    assert _untouched(guards), "a store behind an output"
    assert torch.equal(runs[0][0], u["dg"]) and torch.equal(runs[1][0], u["dg"]), "dg differs from the unfused chain"
    ops_ = R.operands(_cpu(u["gl"]).view(B, T, C), _cpu(u["dc"]).view(B, T, C), K, BF)
    _report(f"fold {tiles} tiles", "unfused", case, R.check_bwd_w(ops_, _cpu(u["dw"]), _cpu(u["db"])))
    for _, dw, db in runs:
        _report(f"fold {tiles} tiles", "fused", case, R.check_bwd_w(ops_, _cpu(dw), _cpu(db)))
    same_runs = torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    same_unfused = torch.equal(runs[0][1], u["dw"]) and torch.equal(runs[0][2], u["db"])
    _NOTES.append(f"fold {R.case_id(case)} ({tiles} tiles): two fused calls equal: {same_runs}; fused equals unfused: {same_unfused}")
    if tiles < 1024:
        assert same_unfused and same_runs, "below 1024 tiles the fused dw / db are the unfused kernel's bit for bit"


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
_ENTRIES = ("dwconv_fwd", "dwconv_fwd_stats", "dwconv_bwd_x", "dwconv_bwd_w", "glu_dwconv_fwd", "conv_bwd_fused")


def _refused(dev, entry, dtype, C, K):
    """one call that must raise: outputs and scratch stay NaN, accumulators keep their start values"""
    from emoasr_amd import lib
    B, T, M, Kw = 2, 5, 10, 33
    x, g = torch.ones(B, T, C, device=dev, dtype=dtype), torch.ones(M, 2 * C, device=dev, dtype=dtype)
    w, vec = torch.ones(C, Kw, device=dev), torch.ones(2, C, device=dev)
    start_w, start_b = torch.randn(C, Kw), torch.randn(C)
    (dw, g0), (db, g1) = _start_out(dev, start_w), _start_out(dev, start_b)
    guards = []
    with pytest.raises(lib.EmoasrHipError):
        if entry == "dwconv_fwd":
            _dw_fwd(dev, x, w, vec[0], K, guards=guards)
        elif entry == "dwconv_fwd_stats":
            _dw_fwd(dev, x, w, vec[0], K, stats=True, guards=guards)
        elif entry == "dwconv_bwd_x":
            _dw_bwd_x(dev, x, w, K, guards)
        elif entry == "dwconv_bwd_w":
            _dw_bwd_w(dev, x, x, K, dw, db, 0, guards)
        elif entry == "glu_dwconv_fwd":
            _fused_fwd(dev, g, B, T, C, K, w, vec[0], True, guards)
        else:
            _fused_bwd(dev, B, T, C, K, x.view(M, C), x.view(M, C), vec[0], vec[1], vec[0], vec[1], vec, g, w, dw, db, guards)
    torch.cuda.synchronize()
    # the outputs and the scratch of the refused call were allocated before it raised: each is the tensor its guard is the tail of
    assert guards and all(bool(torch.isnan(gd._base).all()) for gd in guards), "a refused call wrote"
    assert _untouched([g0, g1]) and torch.equal(dw.cpu(), start_w) and torch.equal(db.cpu(), start_b), "an accumulator changed in a refused call"


@pytest.mark.parametrize("K", [0, 30, 33])
@pytest.mark.parametrize("entry", _ENTRIES)
def test_refuses_unsupported_tap_counts(dev, entry, K):
    for dtype in (BF,) if entry in ("glu_dwconv_fwd", "conv_bwd_fused") else (F32, BF):
        _refused(dev, entry, dtype, 16, K)


@pytest.mark.parametrize("what", ["f32", "C=12"])
@pytest.mark.parametrize("entry", ["glu_dwconv_fwd", "conv_bwd_fused"])
def test_fused_entries_refuse_f32_and_c_not_a_multiple_of_8(dev, entry, what):
    if what == "f32":
        _refused(dev, entry, F32, 16, 31)
    else:
        _refused(dev, entry, BF, 12, 31)
