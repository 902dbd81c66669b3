"""LayerNorm and BatchNorm + Swish as the C ABI (include/emoasr_hip.h) defines them, restated in plain torch on the CPU: in float64
as the reference of tests/test_norm_kernels_gpu.py and in float32 as its error model; pinned against torch.autograd by
tests/test_norm_ref_cpu.py.  Nothing here is taken from the kernels' text: the formulas are the operations', the case tables list the
shapes at which csrc/layernorm.hip and csrc/convmodule.hip change path (the dispatch conditions are quoted in the GPU module).

  ln_fwd        y = (x - mean) rstd gamma + beta; mean = sum x / N, rstd = 1 / sqrt(sum (x - mean)^2 / N + eps): two passes, the
                biased variance, eps inside the root
  ln_bwd        dx = dres + rstd (g dy - mean_N(g dy) - xh mean_N(g dy xh)), dgamma = sum_rows dy xh, dbeta = sum_rows dy, on the
                mean / rstd HANDED IN (as the kernel takes them: forward error does not enter the backward's bound)
  bn_stats      mean, biased var over the M rows; running = (1 - momentum) running + momentum (mean | UNBIASED var); at M = 1 the
                unbiased estimate is 0 / 0 and the running variance takes the biased one (0), the rule of both statistics kernels
  bn_swish_fwd  z = swish(gamma (y - mean) / sqrt(var + eps) + beta), swish(t) = t sigmoid(t)
  bn_swish_bwd  dbn = dz swish'(bn); dy = gamma invstd (dbn - mean_M(dbn) - xh mean_M(dbn xh)); dbeta = sum dbn, dgamma = sum dbn xh

Inputs are seeded per case and rounded to the kernel's dtype BEFORE anyone sees them: the reference, the model and the kernel get
identical operands (gamma, beta, the statistics and eps are float32 in the ABI and are rounded to float32).

The float32 model evaluates the same formulas in float32 with SEQUENTIAL sums (a plain loop: the order with the largest rounding
error among the usual ones, so e32 below is not flattered by a library's blocked summation).  e32 = the model's largest error on the
same case and tensor.  Bounds (the suite's convention: tests/test_ctc_loss_gpu.py, tests/lstm_ref.py; none from the kernels):
  element outputs (y, z, dx, dy)      max(4 e32, 1e-6 (1 + |ref|)), + 2^-8 |ref| for a bf16 output (its worst rounding)
  mean, rstd, the BN statistics       max(4 e32, 1e-6 (1 + |ref|))
  column sums (dgamma, dbeta, means)  R 2^-24 sum_rows |term| + max(4 e32, 1e-6 (1 + |ref|)): R rows added in float32 in ANY order
                                      are within (R - 1) u sum |term| of the exact sum (u = 2^-24); |term| per column in float64;
                                      ref = start + sum where the operation accumulates
  bit-identical, NaN guards, refusals, untouched outputs: exact.

Mutants (MUTANTS: one formula / indexing error each) enter the float32 model through the `tap` hook of the functions below and never
appear in the reference text; tests/test_norm_ref_cpu.py shows each leaving the bounds on a named case of the tables."""
import zlib
from types import SimpleNamespace

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
P8 = 2.0 ** -8          # bf16's worst relative rounding error
U24 = 2.0 ** -24        # float32's


def _no_tap(point, v, **ctx):
    """the hook of the functions below: the reference and the model leave every value alone, a mutant returns another at its point"""
    return v


def _sum(t, dim):
    """float64: torch's sum; float32: one element after the other, in float32"""
    if t.dtype == F64:
        return t.sum(dim)
    t = t.movedim(dim, 0).contiguous()
    s = torch.zeros_like(t[0])
    for k in range(t.shape[0]):
        s = s + t[k]
    return s


def f32_of(v):
    """a Python float as the ABI's `float` argument carries it"""
    return float(torch.tensor(v, dtype=F32))


# ---- the operations -----------------------------------------------------------------------------------------------------------------
def ln_fwd(x, gamma, beta, eps, tap=_no_tap):
    N = x.shape[-1]
    mean = _sum(tap("ln_stat_in", x), -1) / N
    d = x - mean[:, None]
    var = tap("ln_var", _sum(tap("ln_stat_in", d * d), -1) / N, x=x, mean=mean, N=N)
    rstd = tap("ln_rstd", 1.0 / torch.sqrt(var + eps), var=var, eps=eps)
    y = tap("rows_out", d * rstd[:, None] * gamma + beta)
    return y, mean, rstd


def ln_bwd(dy, x, gamma, mean, rstd, dres, tap=_no_tap):
    """-> dx, dgamma, dbeta (the sums alone, nothing accumulated), and the per-column sum |term| of both sums"""
    N = x.shape[-1]
    xh = (x - mean[:, None]) * rstd[:, None]
    gy = dy * gamma
    s1 = _sum(gy, -1) / N
    s2 = tap("ln_s2", _sum(gy * xh, -1) / N)
    dx = rstd[:, None] * (gy - s1[:, None] - xh * s2[:, None])
    if dres is not None:
        dx = dx + tap("ln_dres", dres)
    tg = tap("col_rows", tap("ln_dgamma_term", dy * xh, gy=gy, xh=xh))
    tb = tap("col_rows", dy)
    return tap("rows_out", dx), _sum(tg, 0), _sum(tb, 0), tg.abs().sum(0), tb.abs().sum(0)


def bn_stats(y, running_mean, running_var, momentum, tap=_no_tap):
    """-> mean, var (biased), new running mean, new running var"""
    M = y.shape[0]
    mean = _sum(y, 0) / M
    d = tap("col_rows", y - mean)
    m2 = _sum(d * d, 0)
    var = m2 / M
    unb = tap("bn_unbiased", m2 / (M - 1) if M > 1 else var, var=var)
    return mean, var, (1 - momentum) * running_mean + momentum * mean, (1 - momentum) * running_var + momentum * unb


def _bn(y, mean, var, gamma, beta, eps):
    xh = (y - mean) / torch.sqrt(var + eps)
    return xh, gamma * xh + beta


def bn_swish_fwd(y, mean, var, gamma, beta, eps, tap=_no_tap):
    _, bn = _bn(y, mean, var, gamma, beta, eps)
    return tap("rows_out", bn * torch.sigmoid(bn))


def bn_swish_bwd(dz, y, mean, var, gamma, beta, eps, tap=_no_tap):
    """-> dy, dgamma, dbeta (the sums alone), the means (mean dbn, mean dbn xh), and the per-column sum |term| of both sums"""
    M = y.shape[0]
    xh, bn = _bn(y, mean, var, gamma, beta, eps)
    s = torch.sigmoid(bn)
    dbn = dz * tap("swish_deriv", s * (1 + bn * (1 - s)), s=s)
    tb, tg = tap("col_rows", dbn), tap("col_rows", dbn * xh)
    sb, sg = _sum(tb, 0), _sum(tg, 0)
    m1, m2 = sb / M, sg / M
    dy = gamma / torch.sqrt(var + eps) * (dbn - tap("bn_m1", m1) - xh * m2)
    return tap("rows_out", dy), sg, sb, m1, m2, tg.abs().sum(0), tb.abs().sum(0)


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
def _e32(m32, ref):
    return float((m32.double() - ref).abs().max()) if ref.numel() else 0.0


def elem_bound(ref, m32, bf16=False):
    b = torch.clamp(1e-6 * (1 + ref.abs()), min=4 * _e32(m32, ref))
    return b + P8 * ref.abs() if bf16 else b


def colsum_bound(ref, m32, rows, abs_terms):
    """ref / m32 include the start value where the operation accumulates"""
    return rows * U24 * abs_terms + elem_bound(ref, m32)


def share(got, ref, bound):
    """worst |got - ref| / bound (every entry of got must be finite)"""
    got = got.double()
    if ref.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), "non-finite value where the operation defines one"
    return float(((got - ref).abs() / bound).max())


# ---- mutants --------------------------------------------------------------------------------------------------------------------------
def _at(points, fn):
    return lambda point, v, **ctx: fn(v, **ctx) if point in points else v


def _one_pass(var, x, mean, N, **ctx):
    return torch.clamp(_sum(x * x, -1) / N - mean * mean, min=0)      # (clamped, as such kernels are: a negative value is a NaN)


def _skip_last_row(t, **ctx):
    t = t.clone()
    t[-1] = 0
    return t


def _skip_tail8(t, **ctx):
    t = t.clone()
    t[:, -8:] = 0
    return t


MUTANTS = {
    None: _no_tap,
    "one_pass_var": _at({"ln_var"}, _one_pass),                                          # E[x^2] - E[x]^2
    "unbiased_ln_var": _at({"ln_var"}, lambda v, N, **ctx: v * N / (N - 1)),
    "eps_outside": _at({"ln_rstd"}, lambda r, var, eps, **ctx: 1.0 / (torch.sqrt(var) + eps)),
    "dx_no_s2": _at({"ln_s2"}, lambda s, **ctx: torch.zeros_like(s)),                    # dx without the xh mean(g dy xh) term
    "dx_no_dres": _at({"ln_dres"}, lambda r, **ctx: torch.zeros_like(r)),
    "dgamma_gdy": _at({"ln_dgamma_term"}, lambda t, gy, xh, **ctx: gy * xh),             # dgamma from g dy instead of dy
    "overwrite": _at({"acc"}, lambda total, s, **ctx: s),                                # the sums stored, not accumulated
    "last_row": _at({"rows_out", "col_rows"}, _skip_last_row),                           # the last row neither written nor summed
    "tail8": _at({"ln_stat_in"}, _skip_tail8),                                           # the last 8 columns of the last chunk left out of the statistics
    "bn_biased_running": _at({"bn_unbiased"}, lambda u, var, **ctx: var),
    "bn_no_m1": _at({"bn_m1"}, lambda m, **ctx: torch.zeros_like(m)),                    # dy without the mean(dbn) term
    "swish_no_x": _at({"swish_deriv"}, lambda d, s, **ctx: s),                           # swish' without the x (1 - sigmoid) term
}


# ---- case tables ----------------------------------------------------------------------------------------------------------------------
LN_N8 = (8, 64, 144, 248, 256, 264, 504, 512, 520, 768, 1016, 1024)       # N % 8 == 0: chunk counts 1 .. 4, both sides of each edge
LN_N4 = (4, 12, 252, 260, 1020)                                           # N % 4 == 0 only: the general kernels
LN_FWD_M = (1, 3, 4, 5, 7, 8, 9, 4096, 4097, 4099, 4104)                   # the 4 (8) rows of a block; both sides of the M > 4096 switch
LN_HARD = ("mean300", "pm1e4", "const_eps12", "const_eps5", "outlier", "gamma0neg")
# (ln_bwd_blocks, M) of the N % 8 == 0 backward: 8 rows in flight per block
LN_BWD_TRIPS = ((64, 512), (64, 513), (64, 519), (64, 1024), (64, 1029), (512, 4097))
LN_BWD_SMALL_M = (1, 7, 8, 9)
LN_BWD_GEN_M = (1, 4, 5, 1024, 1025, 1029)                                 # the general kernel: either side of 256 blocks x 4 rows


def _uniq(cases):
    out = []
    for c in cases:
        if c not in out:
            out.append(c)
    return out


# ("fwd", family, M, N, kind, eps)
LN_FWD_CASES = _uniq(
    [("fwd", "width", M, N, "randn", 1e-5) for M in (5, 4097) for N in LN_N8 + LN_N4]
    + [("fwd", "rows", M, N, "randn", 1e-12) for N in (264, 1020) for M in LN_FWD_M]
    + [("fwd", "hard", 9, N, kind, 1e-12 if kind == "const_eps12" else 1e-5) for N in (264, 1020) for kind in LN_HARD])
# ("bwd", family, M, N, kind, ln_bwd_blocks)
LN_BWD_CASES = _uniq(
    [("bwd", "width", M, N, "randn", 64) for M in (9, 519) for N in LN_N8]
    + [("bwd", "width", M, N, "randn", 64) for M in (5, 1029) for N in LN_N4]
    + [("bwd", "trips", M, N, "randn", blk) for N in (264, 1024) for blk, M in LN_BWD_TRIPS]
    + [("bwd", "rows", M, 264, "randn", 64) for M in LN_BWD_SMALL_M]
    + [("bwd", "rows", M, N, "randn", 64) for N in (260, 1020) for M in LN_BWD_GEN_M]
    # the immediate fold at nblk = cdiv(M, 8) = 1, 31, 32, 33, 65, 255, 256, 512: gridDim.y = min(8, nblk / 32) of 1, 2, 7 and 8 with
    # slices that do not divide nblk; 2 N = 144 columns: the fold's third column block is partial
    + [("bwd", "finalize", M, 72, "randn", 512) for M in (8, 248, 256, 264, 520, 2040, 2048, 4096)]
    + [("bwd", "hard", 9, N, kind, 64) for N in (264, 1020) for kind in LN_HARD])
LN_CASES = LN_FWD_CASES + LN_BWD_CASES

BN_HARD = ("sat", "near0", "zero_var")
# ("stats", M, C, kind) | ("fwd", M, C, kind) | ("bwd", M, C, kind) | ("conv", B, T, C, K)
BN_STATS_CASES = ([("stats", M, C, "randn") for M in (1, 2, 63, 64, 65, 129) for C in (8, 12, 144, 256, 264, 520)]
                  + [("stats", 129, 264, "mean50")])
BN_FWD_CASES = ([("fwd", M, C, "randn") for M in (1, 17, 901) for C in (8, 12, 144, 256, 264)]
                + [("fwd", 17, C, kind) for C in (12, 264) for kind in BN_HARD])
# one case per forward form whose work items exceed the 8192 x 256 threads of the largest grid: the grid-stride loop's second trip
# (the 8-wide form counts groups of 8 channels, in bf16: 8192 * 256 + 3 rows of C = 8; the scalar form elements: C = 12, f32)
BN_FWD_BIG_CASES = [("fwd", 8192 * 256 + 3, 8, "randn"), ("fwd", 174763, 12, "randn")]
BN_BWD_CASES = ([("bwd", M, C, "randn") for M in (1, 7, 15, 16, 17, 63, 64, 65) for C in (8, 144, 256, 264, 520)]
                + [("bwd", 4097, C, "randn") for C in (8, 264)]
                + [("bwd", 17, 264, kind) for kind in BN_HARD])
BN_CONV_CASES = [("conv", B, T, 24, 31) for B, T in ((1, 1), (1, 31), (1, 32), (2, 33), (3, 65), (70, 33))] + [("conv", 2, 33, 1024, 7)]
BN_CASES = BN_STATS_CASES + BN_FWD_CASES + BN_FWD_BIG_CASES + BN_BWD_CASES + BN_CONV_CASES
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def case_id(case):
    return "-".join(str(v) for v in case)


def dtype_of(name):
    return {"f32": F32, "bf16": BF}[name]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _rt(t, dtype):
    """rounded to the kernel's dtype, held in float32"""
    return t.to(dtype).float()


def ln_inputs(case, dtype):
    """x, dy, dres rounded to `dtype`; gamma / beta float32; mean / rstd: the float64 statistics of x rounded to float32 (what the
    backward is handed); dg0 / db0: the non-zero values dgamma / dbeta start from"""
    _, family, M, N, kind, last = case
    g = _gen(case, str(dtype))
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(M, N) * 2 + 0.5
    gamma, beta = 1 + 0.3 * rn(N), 0.3 * rn(N)
    if kind == "mean300":
        x = 300 + 0.05 * rn(M, N)
    elif kind == "pm1e4":
        x = 1e4 * torch.sign(rn(M, N))
    elif kind in ("const_eps12", "const_eps5"):
        # multiples of 2^-2 below 2^4: every partial sum of a row, in any order, is exact in float32 and so is the mean -- the
        # variance is exactly zero for a two-pass kernel, and rstd = 1 / sqrt(eps) (1e6 under eps 1e-12)
        x = (torch.arange(M) % 7 - 3.25)[:, None].expand(M, N).clone()
    elif kind == "outlier":
        x = 1e-3 * rn(M, N)
        x[M // 2, N // 3] = 1e4
    elif kind == "gamma0neg":
        gamma[::3] = 0.0
        gamma[1::3] = -gamma[1::3].abs() - 0.1
    x = _rt(x, dtype)
    eps = f32_of(last if case[0] == "fwd" else (1e-12 if kind == "const_eps12" else 1e-5))
    _, mean, rstd = ln_fwd(x.double(), gamma.double(), beta.double(), eps)
    return SimpleNamespace(case=case, dtype=dtype, M=M, N=N, x=x, gamma=gamma.float(), beta=beta.float(), eps=eps,
                           dy=_rt(rn(M, N), dtype), dres=_rt(rn(M, N), dtype), mean=mean.float(), rstd=rstd.float(),
                           dg0=rn(N), db0=rn(N))


def bn_inputs(case, dtype):
    """y, dz rounded to `dtype`; the training statistics handed to bn_swish_fwd / bwd are the float64 ones of y rounded to float32"""
    _, M, C, kind = case
    g = _gen(case, str(dtype))
    rn = lambda *s: torch.randn(*s, generator=g)
    y = rn(M, C) * 1.5 + 0.3 * rn(C)
    gamma, beta = 1 + 0.3 * rn(C), 0.3 * rn(C)
    if kind == "mean50":
        y = 50 + 0.01 * rn(M, C)
    elif kind == "sat":          # pre-activations gamma xh + beta at +-20: the sigmoid saturated on both sides
        gamma, beta = 0.01 * rn(C), 20.0 * torch.sign(rn(C))
    elif kind == "near0":
        gamma, beta = 1e-3 * rn(C), 1e-4 * rn(C)
    elif kind == "zero_var":     # every third column constant (sums of multiples of 2^-2: exact in any order)
        y[:, ::3] = (torch.arange(C)[::3] % 7 - 3.25)
    y = _rt(y, dtype)
    rm0, rv0 = rn(C), torch.rand(C, generator=g) + 0.5
    momentum, eps = f32_of(BN_MOMENTUM), f32_of(BN_EPS)
    mean, var, _, _ = bn_stats(y.double(), rm0.double(), rv0.double(), momentum)
    return SimpleNamespace(case=case, dtype=dtype, M=M, C=C, y=y, gamma=gamma.float(), beta=beta.float(), eps=eps, momentum=momentum,
                           dz=_rt(rn(M, C), dtype), mean=mean.float(), var=var.float(), rm0=rm0, rv0=rv0, dg0=rn(C), db0=rn(C))


def conv_inputs(case, dtype):
    _, B, T, C, K = case
    g = _gen(case, str(dtype))
    rn = lambda *s: torch.randn(*s, generator=g)
    return SimpleNamespace(case=case, dtype=dtype, x=_rt(rn(B, T, C), dtype), w=rn(C, K) * 0.2, bias=rn(C), rm0=rn(C),
                           rv0=torch.rand(C, generator=g) + 0.5, momentum=f32_of(BN_MOMENTUM))


# ---- evaluation in a dtype, the model's outputs in kernel form, and the checks ----------------------------------------------------------
def _to(dt, *ts):
    return [None if t is None else t.to(dt) for t in ts]


def _out(t, dtype):
    """a stored element output: rounded to the kernel's dtype"""
    return t.to(dtype).float()


def _acc(tap, start, s):
    return tap("acc", start + s, s=s)


def _memo(inp, key, tap, fn):
    """the untapped evaluations are computed once per input set and shared by every check of it (never modified)"""
    if tap is not _no_tap:
        return fn()
    memo = inp.__dict__.setdefault("_memo", {})
    if key not in memo:
        memo[key] = fn()
    return memo[key]


def eval_ln_fwd(inp, dt, tap=_no_tap):
    return _memo(inp, ("ln_fwd", dt), tap, lambda: ln_fwd(*_to(dt, inp.x, inp.gamma, inp.beta), inp.eps, tap=tap))


def eval_ln_bwd(inp, dt, dres=True, tap=_no_tap):
    return _memo(inp, ("ln_bwd", dt, dres), tap,
                 lambda: ln_bwd(*_to(dt, inp.dy, inp.x, inp.gamma, inp.mean, inp.rstd, inp.dres if dres else None), tap=tap))


def model_ln_fwd(inp, mutant=None):
    """the float32 model in kernel form: y as stored, mean, rstd"""
    y, mean, rstd = eval_ln_fwd(inp, F32, MUTANTS[mutant])
    return _out(y, inp.dtype), mean, rstd


def model_ln_bwd(inp, mutant=None, dres=True):
    """dx as stored, dgamma / dbeta after the accumulation into dg0 / db0"""
    tap = MUTANTS[mutant]
    dx, dg, db, _, _ = eval_ln_bwd(inp, F32, dres, tap)
    return _out(dx, inp.dtype), _acc(tap, inp.dg0, dg), _acc(tap, inp.db0, db)


def check_ln_fwd(inp, y, mean, rstd):
    """outputs (CPU tensors) against the float64 reference -> worst share of the bound per tensor"""
    ref, m32 = eval_ln_fwd(inp, F64), eval_ln_fwd(inp, F32)
    res = {"y": share(y, ref[0], elem_bound(ref[0], m32[0], inp.dtype == BF))}
    if mean is not None:
        res["mean"] = share(mean, ref[1], elem_bound(ref[1], m32[1]))
        res["rstd"] = share(rstd, ref[2], elem_bound(ref[2], m32[2]))
    return res


def check_ln_bwd(inp, dx, dgamma=None, dbeta=None, dres=True):
    """dgamma / dbeta: the buffers after the call, which started from inp.dg0 / inp.db0"""
    ref, m32 = eval_ln_bwd(inp, F64, dres), eval_ln_bwd(inp, F32, dres)
    res = {"dx": share(dx, ref[0], elem_bound(ref[0], m32[0], inp.dtype == BF))}
    for name, got, k, start in (("dgamma", dgamma, 1, inp.dg0), ("dbeta", dbeta, 2, inp.db0)):
        if got is not None:
            res[name] = share(got, start.double() + ref[k], colsum_bound(start.double() + ref[k], start + m32[k], inp.M, ref[k + 2]))
    return res


def eval_bn_stats(inp, dt, tap=_no_tap):
    return bn_stats(*_to(dt, inp.y, inp.rm0, inp.rv0), inp.momentum, tap=tap)


def check_bn_stats(inp, mean, var, rm, rv, y=None):
    """y: the rows the statistics were taken of, when they are not inp.y (the convolution's own output)"""
    if y is not None:
        inp = SimpleNamespace(y=y, rm0=inp.rm0, rv0=inp.rv0, momentum=inp.momentum)
    ref, m32 = eval_bn_stats(inp, F64), eval_bn_stats(inp, F32)
    return {k: share(got, ref[i], elem_bound(ref[i], m32[i])) for i, (k, got) in
            enumerate((("mean", mean), ("var", var), ("run_mean", rm), ("run_var", rv)))}


def model_bn_stats(inp, mutant=None):
    return eval_bn_stats(inp, F32, MUTANTS[mutant])


def eval_bn_fwd(inp, dt, tap=_no_tap):
    return _memo(inp, ("bn_fwd", dt), tap, lambda: bn_swish_fwd(*_to(dt, inp.y, inp.mean, inp.var, inp.gamma, inp.beta), inp.eps, tap=tap))


def model_bn_fwd(inp, mutant=None):
    return _out(eval_bn_fwd(inp, F32, MUTANTS[mutant]), inp.dtype)


def check_bn_fwd(inp, z):
    ref, m32 = eval_bn_fwd(inp, F64), eval_bn_fwd(inp, F32)
    return {"z": share(z, ref, elem_bound(ref, m32, inp.dtype == BF))}


def eval_bn_bwd(inp, dt, tap=_no_tap):
    return _memo(inp, ("bn_bwd", dt), tap,
                 lambda: bn_swish_bwd(*_to(dt, inp.dz, inp.y, inp.mean, inp.var, inp.gamma, inp.beta), inp.eps, tap=tap))


def model_bn_bwd(inp, mutant=None):
    """dy as stored, dgamma / dbeta after the accumulation, the two means"""
    tap = MUTANTS[mutant]
    dy, sg, sb, m1, m2, _, _ = eval_bn_bwd(inp, F32, tap)
    return _out(dy, inp.dtype), _acc(tap, inp.dg0, sg), _acc(tap, inp.db0, sb), m1, m2


def check_bn_bwd(inp, dy=None, dgamma=None, dbeta=None, m1=None, m2=None):
    ref, m32 = eval_bn_bwd(inp, F64), eval_bn_bwd(inp, F32)
    res = {}
    if dy is not None:
        res["dy"] = share(dy, ref[0], elem_bound(ref[0], m32[0], inp.dtype == BF))
    for name, got, k, start in (("dgamma", dgamma, 1, inp.dg0), ("dbeta", dbeta, 2, inp.db0)):
        if got is not None:
            res[name] = share(got, start.double() + ref[k], colsum_bound(start.double() + ref[k], start + m32[k], inp.M, ref[k + 4]))
    # the means are column sums over M rows divided by M: the sum's bound / M, + the division's rounding inside the 1e-6 term
    for name, got, k, ka in (("m1", m1, 3, 6), ("m2", m2, 4, 5)):
        if got is not None:
            res[name] = share(got, ref[k], colsum_bound(ref[k], m32[k], inp.M, ref[ka] / inp.M))
    return res
