"""The Conv2d subsampling front end (two 3 x 3, stride-2 convolutions, channels-last) as the C ABI (include/emoasr_hip.h) defines
it, restated in plain torch on the CPU: in float64 as the reference of tests/test_frontend_kernels_gpu.py and in float32 with
SEQUENTIAL sums (norm_ref._sum) as its error model; pinned against torch.nn.functional.conv2d + autograd by
tests/test_frontend_ref_cpu.py.  Nothing here is taken from the kernels' text: the formulas are the operations', the case tables
list the shapes at which the entry points change path (the dispatch conditions are quoted in the GPU module).

  T1 = (T - 3) // 2 + 1, F1 = (F - 3) // 2 + 1 (an even T or F leaves its last row / column unread); T2, F2 the same of T1, F1
  conv1_fwd        y1[b,t1,f1,c] = relu(b1[c] + sum_{kh,kw} w1[c, kh*3+kw] x[b, 2t1+kh, 2f1+kw])
  conv1_wgrad      dw1[c, kh*3+kw] (+)= sum_{b,t1,f1} dy1[b,t1,f1,c] x[b, 2t1+kh, 2f1+kw], db1[c] (+)= sum dy1; + sum |term|
  conv2_fwd        y2[(b,t2,f2), n] = act(alpha sum_{kh,kw,c} y1[b, 2t2+kh, 2f2+kw, c] W[n, (kh,kw,c)] + bias[n])
  conv2_dgrad      dy1[b,t1,f1,c] = [y1 > 0] sum_{kh,kw,n} dy2[b, (t1-kh)/2, (f1-kw)/2, n] W[n, (kh,kw,c)] over the taps whose source
                   index is even and inside [0, T2) x [0, F2); layout "w": W [C, 9C] as (n; kh, kw, c), layout "wt": [C, 9C] as
                   (c; kh, kw, n) (the _kc entries)
  col2im           the same gather-sum of a given dcol [(b,t2,f2), (kh,kw,c)]
  conv2_wgrad      dW[n, (kh,kw,c)] (+)= sum_rows dy2[row, n] y1[b, 2t2+kh, 2f2+kw, c], dbias[n] (+)= sum_rows dy2; over one or
                   several segments (each its own B and T1) as ONE sum
  conv2_dgrad_w1   conv1_wgrad of the dy1 that conv2_dgrad (layout "wt") stores: dy1 ROUNDED TO bf16

Operands are seeded per case and rounded to the call's dtype BEFORE anyone sees them: the reference, the model and the kernel get
identical operands.  x, w1, b1, the biases and the start values of every accumulator are float32.

(a) INTEGER cases.  Operands are small integers that bf16 holds exactly; every partial sum of every output is an integer below
2^24, so every float32 summation order gives the float64 result exactly: equality.  bf16 OUTPUTS are made bf16-exact by
construction: sparse_w2 has nine non-zeros of +-1 / +-2 per output channel n, one per tap, at c = (n + 37 tap) mod C -- every
(tap, c) is met once across n, for a fixed (tap, c) exactly one n is non-zero -- so with activations in [-7, 7] a forward sum is at
most 9 * 2 * 7 = 126 (+ a bias of at most 4) and a data-gradient sum at most 4 * 2 * 7 = 56 in magnitude.  assert_exact states the
precondition (stored values bf16-exact, sum |term| < 2^24); tests/test_frontend_ref_cpu.py runs it over every table.

(b) randn cases, bounds from tests/norm_ref.py (none from a kernel's output).  An element that is a reduction of R products added
in float32 in ANY order:  R 2^-24 sum |term| + elem_bound(ref, e32, bf16) = colsum_bound with the reduction length as rows
(R = 9 conv1, 9C conv2 forward, ntap C data gradient and ntap col2im with ntap = (2 - t1 % 2)(2 - f1 % 2) of the element's
parity class -- class_taps --, B T2 F2 weight gradients, B T1 F1 dw1 / db1).  ReLU is 1-Lipschitz; [y1 > 0] is decided on an operand.

f32x3 (dtype code 2; csrc/gemm.hip SplitCfg / split_store4, csrc/mma.h Mma<f32s>): x = hi + lo + r with hi = bf16(x),
lo = bf16(x - hi), both round-to-nearest to bf16's 8 significand bits: |x - hi| <= 2^-8 |x|, |r| <= 2^-8 |x - hi| <= 2^-16 |x|.
The kernels keep ah bh + ah bl + al bh and DROP al bl.  a b - kept = al bl + ra b + a rb - (ra rb + ra bl + al rb), so
|a b - kept| <= (2^-16 + 2^-16 + 2^-16)(1 + 2^-7) |a b|:  c = F32X3_C = 3.03 in  c 2^-16 sum |term|.
(tests/test_frontend_ref_cpu.py recomputes the constant on random operands: 1.8 is met.)

conv2_dgrad_w1: colsum_bound over B T1 F1 rows of the terms dy1r x (dy1r = the float64 dy1 rounded to bf16)
+ 2^-8 sum |dy1_ref x| (the kernel's dy1 is rounded where the kernel chooses) + sum bound(dy1) |x| (the data gradient's own bound
before rounding, through the linear sum).

Mutants (MUTANTS: one formula / indexing error each) enter the float32 model through the `tap` hook and never appear in the
reference text; tests/test_frontend_ref_cpu.py shows each leaving the bound, or breaking equality, on a named case -- but
fold_no_round, which the 2^-8 sum |dy1 x| term admits by design and no integer case can see (dy1 is bf16-exact there)."""
from types import SimpleNamespace

import torch

from tests.norm_ref import BF, F32, F64, P8, _at, _gen, _no_tap, _rt, _sum, colsum_bound, share

F32X3 = "f32x3"                 # float32 buffers, split products: a dtype NAME of the tables below (storage float32)
F32X3_C = 3.03
DTYPES = {"f32": F32, "bf16": BF, "f32x3": F32}
ACT_NONE, ACT_RELU = 0, 1


def out_len(n):
    return (n - 3) // 2 + 1


def cdiv(a, b):
    return -(-a // b)


# ---- the operations -----------------------------------------------------------------------------------------------------------------
def _ti(kh, kw, tap):
    return tap("tap_index", kh * 3 + kw, kh=kh, kw=kw)


def _win(a, n1, m1, kh, kw, tap):
    """a[b, 2 i + kh, 2 j + kw, ...] for i < n1, j < m1"""
    s = tap("stride", 2)
    r = tap("row0", 0, H=a.shape[1], n1=n1)
    return a[:, r + kh:r + kh + s * (n1 - 1) + 1:s, kw:kw + s * (m1 - 1) + 1:s]


def _taps():
    return [(kh, kw) for kh in range(3) for kw in range(3)]


def conv1_fwd(x, w1, b1, tap=_no_tap):
    """x [B, T, F], w1 [C, 9], b1 [C] -> y1 [B, T1, F1, C], sum |term|"""
    B, T, F = x.shape
    T1, F1, C = out_len(T), out_len(F), w1.shape[0]
    terms = torch.stack([b1.expand(B, T1, F1, C)]
                        + [w1[:, _ti(kh, kw, tap)] * _win(x, T1, F1, kh, kw, tap)[..., None] for kh, kw in _taps()])
    return torch.relu(_sum(terms, 0)), terms.abs().sum(0)


def _rows_dot_t(d, xs):
    """d [R, C], xs [R, J] -> sum_r d[r, :, None] xs[r, None, :] as [C, J]; float32: row after row"""
    if d.dtype == F64:
        return d.t() @ xs
    s = torch.zeros(d.shape[1], xs.shape[1], dtype=d.dtype)
    for r in range(d.shape[0]):
        s = s + d[r, :, None] * xs[r, None, :]
    return s


def conv1_wgrad(x, dy1, tap=_no_tap):
    """x [B, T, F], dy1 [B, T1, F1, C] -> dw1 [C, 9], db1 [C] (the sums alone), and sum |term| of both"""
    B, T1, F1, C = dy1.shape
    cols = [None] * 9
    for kh, kw in _taps():
        cols[_ti(kh, kw, tap)] = _win(x, T1, F1, kh, kw, tap)
    xs = torch.stack(cols + [torch.ones_like(cols[0])], -1).reshape(B * T1 * F1, 10)
    d = tap("w1_rows", dy1.reshape(B * T1 * F1, C))
    s, a = _rows_dot_t(d, xs), d.abs().double().t() @ xs.abs().double()
    return s[:, :9].contiguous(), s[:, 9].contiguous(), a[:, :9].contiguous(), a[:, 9].contiguous()


def im2col(y1, tap=_no_tap):
    """y1 [B, T1, F1, C] -> [B T2 F2, 9 C] as (kh, kw, c)"""
    B, T1, F1, C = y1.shape
    T2, F2 = out_len(T1), out_len(F1)
    cols = [None] * 9
    for kh, kw in _taps():
        cols[_ti(kh, kw, tap)] = _win(y1, T2, F2, kh, kw, tap)
    return torch.stack(cols, 3).reshape(B * T2 * F2, 9 * C)


def _dot(a, b):
    """a [M, K], b [N, K] -> [M, N]; float32: one k after the other"""
    if a.dtype == F64:
        return a @ b.t()
    s = torch.zeros(a.shape[0], b.shape[0], dtype=a.dtype)
    for k in range(a.shape[1]):
        s = s + a[:, k, None] * b[None, :, k]
    return s


def conv2_fwd(y1, w, bias, act=ACT_RELU, alpha=1.0, tap=_no_tap):
    """-> y2 [B T2 F2, N], sum |term|"""
    col = im2col(y1, tap)
    v = alpha * _dot(col, w)
    a = abs(alpha) * (col.abs().double() @ w.abs().double().t())
    if bias is not None:
        v, a = v + bias, a + bias.abs().double()
    return (torch.relu(v) if act == ACT_RELU else v), a


def _wtap(w, layout, j, C, tap):
    """the [N, C] slice of tap j = kh*3+kw"""
    layout = tap("layout", layout)
    if layout == "w":
        return w[:, j * C:(j + 1) * C]
    return w[:, j * C:(j + 1) * C].t()


def _src(n1, n2, k, tap):
    """per output index i < n1 of tap k: the source index (i - k) / 2 and whether it exists"""
    d = torch.arange(n1) - k
    ok = tap("parity", (d >= 0) & (d % 2 == 0) & (d // 2 < n2), d=d, n2=n2)
    return torch.clamp(d // 2, 0, n2 - 1), ok


def _gather(P, T1, F1, kh, kw, tap):
    """P [B, T2, F2, C] of tap (kh, kw) -> its contribution to [B, T1, F1, C]"""
    _, T2, F2, _ = P.shape
    ti, tok = _src(T1, T2, kh, tap)
    fi, fok = _src(F1, F2, kw, tap)
    g = P[:, ti][:, :, fi]
    return g * (tok[:, None] & fok[None, :])[None, :, :, None].to(P.dtype)


def conv2_dgrad(dy2, w, y1, layout="w", tap=_no_tap):
    """dy2 [B T2 F2, N], y1 [B, T1, F1, C] -> dy1 [B, T1, F1, C], sum |term|"""
    B, T1, F1, C = y1.shape
    T2, F2 = out_len(T1), out_len(F1)
    s, a = torch.zeros_like(y1), torch.zeros(B, T1, F1, C, dtype=F64)
    for kh, kw in _taps():
        wj = _wtap(w, layout, _ti(kh, kw, tap), C, tap)                       # [N, C]
        s = s + _gather(_dot(dy2, wj.t()).reshape(B, T2, F2, C), T1, F1, kh, kw, tap)
        a = a + _gather((dy2.abs().double() @ wj.abs().double()).reshape(B, T2, F2, C), T1, F1, kh, kw, _no_tap)
    live = (y1 > 0).to(s.dtype)
    return s * live, a * live.double()


def col2im(dcol, y1, tap=_no_tap):
    B, T1, F1, C = y1.shape
    T2, F2 = out_len(T1), out_len(F1)
    s, a = torch.zeros_like(y1), torch.zeros(B, T1, F1, C, dtype=F64)
    for kh, kw in _taps():
        j = _ti(kh, kw, tap)
        P = dcol[:, j * C:(j + 1) * C].reshape(B, T2, F2, C)
        s = s + _gather(P, T1, F1, kh, kw, tap)
        a = a + _gather(P.abs().double(), T1, F1, kh, kw, _no_tap)
    live = (y1 > 0).to(s.dtype)
    return s * live, a * live.double()


def conv2_wgrad(segs, tap=_no_tap):
    """segs: [(dy2 [B T2 F2, N], y1 [B, T1, F1, C]), ...] -> dW [N, 9C], dbias [N] (the sums alone) and sum |term| of both"""
    d = tap("w2_rows", torch.cat([dy2 for dy2, _ in segs], 0))
    col = torch.cat([im2col(y1, tap) for _, y1 in segs], 0)
    ones = torch.ones(col.shape[0], 1, dtype=col.dtype)
    s = _rows_dot_t(d, torch.cat([col, ones], 1))
    a = d.abs().double().t() @ torch.cat([col, ones], 1).abs().double()
    return s[:, :-1].contiguous(), s[:, -1].contiguous(), a[:, :-1].contiguous(), a[:, -1].contiguous()


def conv2_dgrad_w1(dy2, wt, y1, x, tap=_no_tap):
    """-> dw1, db1, sum |term| of both (of the ROUNDED dy1), and the unrounded dy1 with its sum |term|"""
    dy1, a1 = conv2_dgrad(dy2, wt, y1, "wt", tap)
    dy1r = tap("fold_round", dy1.to(BF).to(dy1.dtype), dy1=dy1)
    return conv1_wgrad(x, dy1r, tap) + (dy1, a1)


# ---- mutants ------------------------------------------------------------------------------------------------------------------------
def _drop_last_rows(d, **ctx):
    """the last 64th of the rows left out of the sum (a fold slice dropped)"""
    d = d.clone()
    d[d.shape[0] - cdiv(d.shape[0], 64):] = 0
    return d


MUTANTS = {
    None: _no_tap,
    "stride1": _at({"stride"}, lambda s, **ctx: 1),                                        # windows one apart
    "tap_order": _at({"tap_index"}, lambda j, kh, kw, **ctx: kw * 3 + kh),                 # (kw, kh) where (kh, kw) is meant
    "no_parity": _at({"parity"}, lambda ok, d, n2, **ctx: (d >= 0) & (d // 2 < n2)),       # odd source offsets rounded down and used
    "last_row": _at({"row0"}, lambda r, H, n1, **ctx: H - (2 * n1 + 1)),                   # windows anchored at the END: an even T reads its last row
    "wt_as_w": _at({"layout"}, lambda layout, **ctx: "w"),                                 # the (c; kh, kw, n) weight read as (n; kh, kw, c)
    "fold_no_round": _at({"fold_round"}, lambda r, dy1, **ctx: dy1),                       # the fold on the unrounded dy1
    "fold_slice": _at({"w1_rows"}, _drop_last_rows),
}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _ints(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def sparse_w2(C, gen):
    """[C, 9C] as (n; kh, kw, c): per n one +-1 / +-2 per tap at c = (n + 37 tap) mod C"""
    w = torch.zeros(C, 9, C)
    n = torch.arange(C)
    for j in range(9):
        v = _ints(gen, 1, 2, C) * (2 * _ints(gen, 0, 1, C) - 1)
        w[n, j, (n + 37 * j) % C] = v
    return w.reshape(C, 9 * C)


def wt_of(w):
    """(n; kh, kw, c) -> (c; kh, kw, n)"""
    N = w.shape[0]
    C = w.shape[1] // 9
    return w.reshape(N, 9, C).permute(2, 1, 0).reshape(C, 9 * N).contiguous()


def _operand(gen, kind, dtype, *shape, lim=7, zeros=False):
    """integers in [-lim, lim], or randn rounded to dtype; zeros: a third of the entries exactly 0 (a ReLU output has them)"""
    t = _ints(gen, -lim, lim, *shape) if kind == "int" else _rt(torch.randn(*shape, generator=gen), dtype)
    if zeros:
        t = t * (torch.rand(*shape, generator=gen) > 1 / 3).float()
    return t


def _start(gen, kind, *shape):
    return _ints(gen, -9, 9, *shape) if kind == "int" else torch.randn(*shape, generator=gen)


def conv1_inputs(case, dname):
    """("c1f" | "c1w", kind, B, T, F, C)"""
    _, kind, B, T, F, C = case
    gen, dtype = _gen(case, dname), DTYPES[dname]
    T1, F1 = out_len(T), out_len(F)
    if kind == "int":
        x, w1, b1 = _ints(gen, -3, 3, B, T, F), _ints(gen, -2, 2, C, 9), _ints(gen, -3, 3, C)
    else:
        x, w1, b1 = torch.randn(B, T, F, generator=gen), torch.randn(C, 9, generator=gen) / 3, torch.randn(C, generator=gen)
    return SimpleNamespace(case=case, kind=kind, dname=dname, dtype=dtype, B=B, T=T, F=F, C=C, T1=T1, F1=F1, x=x, w1=w1, b1=b1,
                           dy1=_operand(gen, kind, dtype, B, T1, F1, C), dw0=_start(gen, kind, C, 9), db0=_start(gen, kind, C))


def conv2_inputs(case, dname):
    """("c2f" | "c2d", kind, B, T1, F1, C): y1 (with exact zeros), dy2, dcol; w sparse (int) or randn / sqrt(9C); bias"""
    _, kind, B, T1, F1, C = case
    gen, dtype = _gen(case, dname), DTYPES[dname]
    T2, F2 = out_len(T1), out_len(F1)
    M = B * T2 * F2
    w = sparse_w2(C, gen) if kind == "int" else _rt(torch.randn(C, 9 * C, generator=gen) * (9 * C) ** -0.5, dtype)
    # dcol: each output takes at most four taps: integers in [-7, 7] keep a bf16 dy1 exact (<= 28)
    return SimpleNamespace(case=case, kind=kind, dname=dname, dtype=dtype, B=B, T1=T1, F1=F1, C=C, T2=T2, F2=F2, M=M,
                           y1=_operand(gen, kind, dtype, B, T1, F1, C, zeros=True), w=w, wt=wt_of(w),
                           bias=_ints(gen, -4, 4, C) if kind == "int" else torch.randn(C, generator=gen),
                           dy2=_operand(gen, kind, dtype, M, C, zeros=True), dcol=_operand(gen, kind, dtype, M, 9 * C))


def wgrad_inputs(case, dname):
    """("c2w", kind, ((B, T1), ...), F1, C): per segment dy2 [B T2 F2, C] and y1 [B, T1, F1, C]; dense operands"""
    _, kind, segs, F1, C = case
    gen, dtype = _gen(case, dname), DTYPES[dname]
    F2 = out_len(F1)
    lim = 7 if kind == "int" else None
    data = [(_operand(gen, kind, dtype, B * out_len(T1) * F2, C, lim=lim, zeros=True), _operand(gen, kind, dtype, B, T1, F1, C, lim=lim))
            for B, T1 in segs]
    return SimpleNamespace(case=case, kind=kind, dname=dname, dtype=dtype, segs=segs, F1=F1, F2=F2, C=C, data=data,
                           rows=sum(d.shape[0] for d, _ in data), dw0=_start(gen, kind, C, 9 * C), db0=_start(gen, kind, C))


def fold_inputs(case, dname="bf16"):
    """("w1", kind, B, T, F, C): x f32 [B, T, F]; y1, dy2 bf16; wt; the accumulators' start values"""
    _, kind, B, T, F, C = case
    gen = _gen(case, dname)
    T1, F1 = out_len(T), out_len(F)
    T2, F2 = out_len(T1), out_len(F1)
    w = sparse_w2(C, gen) if kind == "int" else _rt(torch.randn(C, 9 * C, generator=gen) * (9 * C) ** -0.5, BF)
    x = _ints(gen, -3, 3, B, T, F) if kind == "int" else torch.randn(B, T, F, generator=gen)
    return SimpleNamespace(case=case, kind=kind, dname=dname, dtype=BF, B=B, T=T, F=F, C=C, T1=T1, F1=F1, T2=T2, F2=F2, x=x,
                           y1=_operand(gen, kind, BF, B, T1, F1, C, zeros=True), wt=wt_of(w),
                           dy2=_operand(gen, kind, BF, B * T2 * F2, C, zeros=True), dw0=_start(gen, kind, C, 9), db0=_start(gen, kind, C))


# ---- evaluation, bounds, exactness ----------------------------------------------------------------------------------------------------
def _memo(inp, key, fn):
    memo = inp.__dict__.setdefault("_memo", {})
    if key not in memo:
        memo[key] = fn()
    return memo[key]


def _to(dt, *ts):
    return [None if t is None else t.to(dt) for t in ts]


def ev(inp, op, dt, tap=_no_tap, **kw):
    """the operation `op` of this input set evaluated in dt (float64: the reference; float32: the model, or a mutant of it)"""
    def fn():
        if op == "c1f":
            return conv1_fwd(*_to(dt, inp.x, inp.w1, inp.b1), tap=tap)
        if op == "c1w":
            return conv1_wgrad(*_to(dt, inp.x, inp.dy1), tap=tap)
        if op == "c2f":
            bias = inp.bias if kw.get("bias", True) else None
            return conv2_fwd(*_to(dt, inp.y1, inp.w, bias), act=kw.get("act", ACT_RELU), alpha=kw.get("alpha", 1.0), tap=tap)
        if op == "c2d":
            layout = kw.get("layout", "w")
            return conv2_dgrad(*_to(dt, inp.dy2, inp.w if layout == "w" else inp.wt, inp.y1), layout=layout, tap=tap)
        if op == "col2im":
            return col2im(*_to(dt, inp.dcol, inp.y1), tap=tap)
        if op == "c2w":
            return conv2_wgrad([tuple(_to(dt, d, y)) for d, y in inp.data[:kw.get("nseg", len(inp.data))]], tap=tap)
        if op == "w1":
            return conv2_dgrad_w1(*_to(dt, inp.dy2, inp.wt, inp.y1, inp.x), tap=tap)
        raise KeyError(op)
    return fn() if tap is not _no_tap else _memo(inp, (op, dt, tuple(sorted(kw.items()))), fn)


def _bf_exact(t):
    return bool((t.to(BF).double() == t.double()).all())


def assert_exact(inp, op, **kw):
    """the precondition of an integer case: operands and every stored value bf16-exact integers, every sum |term| below 2^24"""
    res = ev(inp, op, F64, **kw)
    n = len(res) // 2 if op != "w1" else 2
    for t in res[:n]:
        assert kw.get("alpha", 1.0) != 1.0 or bool((t == t.round()).all())
    for a in res[n:2 * n]:
        assert float(a.max()) < 2 ** 24 - 2 ** 10, (inp.case, op, float(a.max()))      # (2^10: room for the start values)
    if op in ("c1f", "c2f", "c2d", "col2im"):
        assert _bf_exact(res[0]) and float(res[0].abs().max()) <= 256, (inp.case, op)
    if op == "w1":
        assert _bf_exact(res[4]) and float(res[4].abs().max()) <= 256, (inp.case, op)    # dy1: the rounding inside the fold is the identity
    return res


def class_taps(T1, F1):
    """[1, T1, F1, 1]: the taps of the parity class of (t1, f1), (2 - t1 % 2)(2 - f1 % 2): 4, 2, 2 or 1"""
    t, f = torch.arange(T1), torch.arange(F1)
    return ((2 - t % 2)[:, None] * (2 - f % 2)[None, :]).double()[None, :, :, None]


def reduce_len(inp, op):
    """the number of products of one output element (a tensor where it differs per element)"""
    return {"c1f": lambda: 9, "c1w": lambda: inp.B * inp.T1 * inp.F1, "c2f": lambda: 9 * inp.C,
            "c2d": lambda: class_taps(inp.T1, inp.F1) * inp.C, "col2im": lambda: class_taps(inp.T1, inp.F1),
            "c2w": lambda: inp.rows, "w1": lambda: inp.B * inp.T1 * inp.F1}[op]()


def bound(inp, op, k, start=None, **kw):
    """-> (reference, bound) of output k of `op` (randn cases); start: the accumulator's start value"""
    ref, m32 = ev(inp, op, F64, **kw), ev(inp, op, F32, **kw)
    n = 2 if op in ("c1w", "c2w", "w1") else 1
    r, m, a = ref[k], m32[k], ref[n + k]
    if start is not None:
        r, m = start.double() + r, start + m
    b = colsum_bound(r, m, reduce_len(inp, op), a)
    if inp.dtype == BF and n == 1 and not kw.get("out_f32", False):
        b = b + P8 * r.abs()                                               # a bf16 element output: its worst rounding
    if inp.dname == F32X3 and op in ("c2f", "c2d", "c2w"):
        b = b + F32X3_C * 2.0 ** -16 * a
    if op == "w1":
        dy1, a1 = ref[4], ref[5]
        dyb = colsum_bound(dy1, m32[4], class_taps(inp.T1, inp.F1) * inp.C, a1)      # the data gradient's bound before its rounding
        b = b + conv1_wgrad(inp.x.double(), P8 * dy1.abs() + dyb)[2 + k]   # sum over rows of (2^-8 |dy1| + bound(dy1)) |x|
    return r, b


def check(inp, op, k, got, start=None, **kw):
    r, b = bound(inp, op, k, start=start, **kw)
    return share(got.reshape(r.shape), r, b)


# ---- the four parity classes of the data gradient (rows and taps follow from the operation; tiles = rows over the tile height) ----
def class_rows(B, T1, F1):
    """rows of the parity classes (pt, pf) in launch order, with their tap counts"""
    return [(B * ((T1 - pt + 1) // 2) * ((F1 - pf + 1) // 2), (2 - pt) * (2 - pf)) for pt in (0, 1) for pf in (0, 1)]


def class_tiles(B, T1, F1, bm):
    return sum(cdiv(m, bm) for m, _ in class_rows(B, T1, F1))


# ---- case tables ----------------------------------------------------------------------------------------------------------------------
def case_id(case):
    return "-".join(str(v).replace(" ", "").replace("(", "").replace(")", "").replace(",", "x") for v in case)


C1F_T = tuple(range(3, 12))      # odd and even T (the unread last row); T1 = 1 .. 5: the pair kernel with and without a second row
C1F_F = (3, 4, 7, 8, 80, 83, 130, 131)
C1F_INT = ([("c1f", "int", 3, T, F, 256) for T in C1F_T for F in C1F_F]
           + [("c1f", "int", 1, T, F, 256) for T in (3, 4, 11) for F in (3, 131)]
           + [("c1f", "int", B, T, F, C) for C in (8, 32, 264, 512) for B, T, F in ((3, 4, 8), (1, 5, 3), (3, 10, 83), (3, 11, 7))])
C1F_RANDN = [("c1f", "randn", 3, 10, 83, 264), ("c1f", "randn", 3, 11, 80, 256), ("c1f", "randn", 1, 7, 131, 8)]

C1W_T1 = (1, 7, 8, 9, 31, 32, 33, 65)      # both sides of the 8 staged rows and of the 32-row chunk; three chunks
C1W_F1 = (1, 7, 8, 9, 63, 64)              # the 8 f1 lanes x 8 positions per lane
# T = 2 T1 + 1 and 2 T1 + 2; F = 2 F1 + 1 and 2 F1 + 2 alternate with T1 + F1
C1W_INT = ([("c1w", "int", 1, 2 * T1 + 1 + p, 2 * F1 + 1 + (T1 + F1 + p) % 2, 256) for T1 in C1W_T1 for F1 in C1W_F1 for p in (0, 1)]
           + [("c1w", "int", 3, 2 * T1 + 1 + p, 2 * F1 + 2 - p, C) for C in (8, 256, 264, 512) for T1, F1, p in ((9, 9, 0), (33, 64, 1))])
C1W_RANDN = [("c1w", "randn", 3, 68, 19, 264), ("c1w", "randn", 1, 19, 130, 256)]

C2F_M = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)      # both sides of the tile heights 64, 128, 192, 256


def _b_of(m):
    return next((b for b in (3, 2, 5) if m % b == 0 and m > b), 1)


# F1 = 3: F2 = 1, M = B T2
C2F_EDGE = [("c2f", "int", _b_of(M), 2 * (M // _b_of(M)) + 1, 3, 256) for M in C2F_M]
C2F_INT = ([("c2f", "int", 2, T1, F1, 256) for T1 in (3, 4, 5, 6) for F1 in (3, 4, 5, 6)] + C2F_EDGE
           + [("c2f", "int", B, T1, F1, C) for C in (32, 64, 128, 512) for B, T1, F1 in ((2, 5, 6), (5, 27, 3))])
C2F_RANDN = [("c2f", "randn", 3, 9, 8, 256), ("c2f", "randn", 2, 6, 5, 64), ("c2f", "randn", 1, 5, 7, 512)]

# one-tap class rows B (T1 // 2) (F1 // 2) with F1 = 3, and heaviest class rows B ceil(T1 / 2) ceil(F1 / 2) with F1 = 3 (x 2) or
# F1 = 5 (x 3) on both sides of 128 / 192 / 256
C2D_ONE = [("c2d", "int", _b_of(m), 2 * (m // _b_of(m)) + 1, 3, 256) for m in (127, 128, 129, 191, 192, 193, 255, 256, 257)]
C2D_HEAVY = ([("c2d", "int", 1, 2 * (m // 2) - 1, 3, 256) for m in (126, 128, 130, 190, 192, 194, 254, 256, 258)]
             + [("c2d", "int", 1, 2 * (m // 3) - 1, 5, 256) for m in (129, 189, 195, 255, 258)])
C2D_INT = ([("c2d", "int", 2, T1, F1, 256) for T1 in range(3, 9) for F1 in range(3, 9)] + C2D_ONE + C2D_HEAVY
           + [("c2d", "int", B, T1, F1, C) for C in (64, 128, 512) for B, T1, F1 in ((2, 5, 6), (3, 8, 7))])
C2D_RANDN = [("c2d", "randn", 3, 8, 7, 256), ("c2d", "randn", 2, 5, 6, 64), ("c2d", "randn", 2, 7, 4, 512)]

# reduction length B T2 F2 over F2 = 1 (F1 = 3) on both sides of 32 / 64 / 128; F2 of one and many carries of the index walk
C2W_K = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)
C2W_INT = ([("c2w", "int", ((_b_of(K), 2 * (K // _b_of(K)) + 1),), 3, 256) for K in C2W_K]
           + [("c2w", "int", ((3, 2 * 9 + 2),), 2 * 37 + 1, 256)]                              # 3 x 9 x 37 = 999 rows: several slices
           + [("c2w", "int", ((2, 2 * T2 + 1),), 2 * F2 + 1 + F2 % 2, 256) for F2, T2 in ((2, 5), (19, 3), (31, 2), (32, 2), (33, 2))]
           + [("c2w", "int", ((2, 9),), 7, C) for C in (128, 512)]
           + [("c2w", "int", ((3, 7),), 41, 128)])                                              # 3 x 3 x 20 = 180 rows
# segments of different B and T1 whose row counts are no multiples of 32 (F2 = 3: rows 3 B T2)
C2W_SEGS = ((3, 9), (1, 5), (2, 11), (1, 3), (5, 7), (2, 4), (1, 13), (3, 6))
C2W_SEG_INT = [("c2w", "int", C2W_SEGS, 7, 256), ("c2w", "int", C2W_SEGS[:3], 8, 512), ("c2w", "int", ((7, 25), (5, 31)), 41, 256)]
C2W_RANDN = [("c2w", "randn", ((3, 9), (2, 11)), 7, 256), ("c2w", "randn", ((3, 7),), 41, 128)]

# the fold: T, F in 7 .. 14 crossed; tile rows of the plan on both sides of the 64 slices of the first fold stage (bm = 128)
W1_INT = ([("w1", "int", 2, T, F, 256) for T in range(7, 15) for F in range(7, 15)]
          + [("w1", "int", 2, 9, 12, 512), ("w1", "int", 3, 14, 13, 512)])
# tile rows at big_bm = 128 -> the smallest B T F that reaches it (four classes exist whenever T1, F1 >= 3: 4 is the least, at
# every small shape above; 1 cannot be reached).  63: slices of one row and an empty last one; 64: one row each; 65: slices of two
# rows, the last 31 empty; 130: three rows per slice, 44 slices used.  The 64-row shape has odd T1 and F1: the last tile row (the
# one-tap class's last rows, the 64th slice) then holds non-zero dy1 -- at an even T1 those rows have no tap and are zeros
W1_TILES = {63: ("w1", "int", 7, 55, 83, 256), 64: ("w1", "int", 10, 55, 59, 256), 65: ("w1", "int", 18, 43, 43, 256),
            130: ("w1", "int", 19, 45, 79, 256)}
W1_RANDN = [("w1", "randn", 3, 13, 14, 256), ("w1", "randn", 2, 9, 23, 512)]
