"""The GLU and depthwise-convolution operations of the Conformer convolution module as the C ABI (include/emoasr_hip.h) defines them,
restated in plain torch on the CPU: in float64 as the reference of tests/test_conv_kernels_gpu.py and in float32 as its error model;
pinned against torch.autograd by tests/test_conv_ref_cpu.py.  Nothing here is taken from the kernels' text: the formulas are the
operations', the case tables list the shapes at which csrc/convmodule.hip and csrc/convfused.hip change path (the dispatch conditions
are quoted in the GPU module).

  glu_fwd         out = a sigmoid(b), a = in[:, :C], b = in[:, C:]
  glu_fwd_masked  the same over [B, T, 2C] with zeros at t >= lens[b]
  glu_bwd         din[:, :C] = d sigmoid(b), din[:, C:] = d a sigmoid(b) (1 - sigmoid(b))
  dwconv_fwd      y[b,t,c] = bias[c] + sum_j w[c,j] x[b, t + j - pad, c], pad = (K - 1) / 2, zeros outside [0, T) of the OWN
                  utterance; the bias is optional
  dwconv_bwd_x    dx[b,t,c] = sum_j w[c, K-1-j] dy[b, t + j - pad, c]: the flipped taps, no bias
  dwconv_bwd_w    dw[c,j] (+)= sum_{b,t} dy[b,t,c] x[b, t + j - pad, c], db[c] (+)= sum_{b,t} dy[b,t,c]; also returns the per-entry
                  sum |term| of both sums, for the bound

Inputs are seeded per case and rounded to the kernel's dtype BEFORE anyone sees them: the reference, the model and the kernel get
identical operands (w, bias and the start values of dw / db are float32 in the ABI).

The float32 model evaluates the same formulas in float32 with SEQUENTIAL sums (norm_ref._sum).  e32 = the model's largest error on
the same case and tensor.  Bounds, imported from tests/norm_ref.py (the suite's convention; none from the kernels):
  element outputs (glu, y, dx)   elem_bound: max(4 e32, 1e-6 (1 + |ref|)), + 2^-8 |ref| for a bf16 output
  dw, db                         colsum_bound: R 2^-24 sum |term| + elem_bound, R = B T rows added in float32 in ANY order;
                                 ref = start + sum where the operation accumulates
  bit-identical, NaN guards, refusals, untouched outputs: exact.

Exact cases (tap_counts, dw_counts): with x = 1, w = 1 and no bias y[t] is the number of taps inside the utterance, an integer <= 31;
with dy = 1 and x = 1, dw[c,j] = B max(0, T - |j - pad|) and db = B T.  Integers below 2^24: every float32 order gives them exactly.

Mutants (MUTANTS: one formula / indexing error each) enter the float32 model through the `tap` hook of the functions below and never
appear in the reference text; tests/test_conv_ref_cpu.py shows each leaving the bounds on a named case of the tables."""
from types import SimpleNamespace

import torch

from tests.norm_ref import BF, F32, F64, _at, _gen, _no_tap, _rt, _sum, colsum_bound, elem_bound, share

EPS = 1e-5          # the BatchNorm between the convolution and its gradient in the chain tests


# ---- the operations -----------------------------------------------------------------------------------------------------------------
def _halves(g, tap):
    C = g.shape[-1] // 2
    return tap("glu_halves", (g[..., :C], g[..., C:]))


def glu_fwd(g, tap=_no_tap):
    a, b = _halves(g, tap)
    return a * torch.sigmoid(b)


def glu_fwd_masked(g, lens, tap=_no_tap):
    """g [B, T, 2C], lens [B]"""
    T = g.shape[1]
    live = torch.arange(T)[None, :] < lens[:, None]
    y = glu_fwd(g, tap)
    return torch.where(live[:, :, None], y, torch.zeros_like(y))


def glu_bwd(g, d, tap=_no_tap):
    a, b = _halves(g, tap)
    s = torch.sigmoid(b)
    return torch.cat([d * s, tap("glu_gate_grad", d * a * s * (1 - s), d=d, s=s)], -1)


def _shift(x, s, tap):
    """x[b, t + s, c], zeros where t + s is outside [0, T) of utterance b"""
    T = x.shape[1]
    out = torch.zeros_like(x)
    lo, hi = max(0, -s), min(T, T - s)
    if hi > lo:
        out[:, lo:hi] = x[:, lo + s:hi + s]
    return tap("shift", out, x=x, s=s)


def _pad(K, tap):
    return tap("pad", (K - 1) // 2, K=K)


def dwconv_fwd(x, w, bias, tap=_no_tap):
    """x [B, T, C], w [C, K], bias [C] or None"""
    K = w.shape[1]
    pad = _pad(K, tap)
    acc = torch.zeros_like(x) if bias is None else bias.expand_as(x).clone()
    for j in range(K):
        acc = acc + w[:, j] * _shift(x, j - pad, tap)
    return acc


def dwconv_bwd_x(dy, w, tap=_no_tap, **ctx):
    K = w.shape[1]
    pad = _pad(K, tap)
    acc = tap("bwd_x_start", torch.zeros_like(dy), **ctx)
    for j in range(K):
        acc = acc + w[:, tap("flip", K - 1 - j, j=j)] * _shift(dy, j - pad, tap)
    return acc


def dwconv_bwd_w(dy, x, K, tap=_no_tap):
    """-> dw [C, K], db [C] (the sums alone, nothing accumulated), and the per-entry sum |term| of both"""
    B, T, C = x.shape
    pad = _pad(K, tap)
    terms = torch.stack([dy * _shift(x, j - pad, tap) for j in range(K)] + [dy], 2)      # [B, T, K + 1, C]
    rows = tap("w_rows", terms).reshape(B * T, K + 1, C)
    s, a = _sum(rows, 0), rows.abs().sum(0)
    return s[:K].t().contiguous(), s[K], a[:K].t().contiguous(), a[K]


# ---- the exact cases ------------------------------------------------------------------------------------------------------------------
def tap_counts(T, K):
    """[T]: the taps of a K-tap window centred on t that lie inside [0, T)"""
    pad = (K - 1) // 2
    t = torch.arange(T)
    return (torch.clamp(t + pad, max=T - 1) - torch.clamp(t - pad, min=0) + 1).float()


def dw_counts(B, T, K):
    """[K]: the frames t of B utterances with t + j - pad inside [0, T)"""
    pad = (K - 1) // 2
    return (B * torch.clamp(T - (torch.arange(K) - pad).abs(), min=0)).float()


# ---- mutants --------------------------------------------------------------------------------------------------------------------------
def _flat_shift(out, x, s, **ctx):
    """the halo read across the utterance boundary: frame t + s of the whole [B T] buffer"""
    B, T, C = x.shape
    f, o = x.reshape(B * T, C), torch.zeros(B * T, C, dtype=x.dtype)
    lo, hi = max(0, -s), min(B * T, B * T - s)
    if hi > lo:
        o[lo:hi] = f[lo + s:hi + s]
    return o.reshape(B, T, C)


def _skip_last_partial_tile(terms, **ctx):
    T = terms.shape[1]
    terms = terms.clone()
    if T % 32:
        terms[:, T - T % 32:] = 0
    return terms


MUTANTS = {
    None: _no_tap,
    "pad15": _at({"pad"}, lambda p, **ctx: 15),                                          # pad fixed at 15 where (K - 1) / 2 is meant
    "no_flip": _at({"flip"}, lambda jj, j, **ctx: j),                                    # the data gradient with the forward's taps
    "halo_leak": _at({"shift"}, _flat_shift),
    "last_tile": _at({"w_rows"}, _skip_last_partial_tile),                               # the last partial 32-frame tile left out of dw / db
    "bwd_x_bias": _at({"bwd_x_start"}, lambda z, bias, **ctx: z + bias),                 # the bias added in the data gradient
    "overwrite": _at({"acc"}, lambda total, s, **ctx: s),                                # dw / db stored, not accumulated
    "glu_swapped": _at({"glu_halves"}, lambda ab, **ctx: (ab[1], ab[0])),
    "glu_gate_no_a": _at({"glu_gate_grad"}, lambda v, d, s, **ctx: d * s * (1 - s)),
}


# ---- case tables: (table, B, T, C, K, kind); each entry is the smallest shape for the mechanism its comment names.  B = 2 unless the
#      table is about B: an utterance-stride error shows -------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


TAPS = [("taps", 2, 70, 24, K, "randn") for K in (
    1,         # pad 0: no halo at all
    3, 5, 7,   # pad 1 .. 3: most of the 31-tap register window holds zero taps
    15, 17,    # either side of the 16-tap split of the fused weight gradient (taps 0 .. 15 | 16 .. 30 on the two thread halves)
    29, 31)]   # the window one short of full, and full
TIME31 = [("time", 2, T, 24, 31, "randn") for T in (
    1, 2, 14, 15,   # the whole utterance inside the halo (T <= pad = 15)
    16, 17,         # the 16-frame half tile of the fused kernels: full, and one frame into the second half
    31, 32, 33,     # the 32-frame tile: one short, full, a second tile of one frame
    47, 48, 49,     # the second tile's half-tile edge
    63, 64, 65,     # the 64-row ring: two tiles, and the third tile's first row lands on the first tile's slot
    96, 97)]        # three full tiles, a fourth of one frame
TIME7 = [("time", 2, T, 24, 7, "randn") for T in (
    1, 3,        # T <= pad = 3
    4,           # the first T past the pad
    32, 33, 64, 65)]   # tile and ring edges at pad 3: the ring keeps slots no tile owns
CHAN_ALL = [("chan", 2, 33, C, 15, "randn") for C in (
    8,            # one 8-channel group: 4 active thread pairs of 128
    16, 24,       # two and three groups
    144,          # a partial channel block
    248, 256,     # one group short of the 256-channel block, and the full block
    264,          # a second channel block of eight channels
    512, 520)]    # two full blocks, a third of eight channels
CHAN_PLAIN = [("chan", 2, 33, C, 15, "randn") for C in (
    1, 12,        # C % 8 != 0, inside one block: the plain kernel in bf16 too
    260,          # bf16 that must fall back from the LDS path, with a second block of four channels
    300)]         # a second block of 44
BATCH = [("batch", B, 33, 24, 31, "edges") for B in (1, 3)]      # |x| = 64 on the first and last frame of every utterance: a halo
#                                                                   that leaks across an utterance boundary is far outside the bound
STRIP_S = (1, 2, 3, 4, 8, 0)      # option conv_strip: tiles per strip; 0 = the library's rule
STRIPS = [("strips", 2, T, C, K, "randn") for T in (
    128,     # 4 tiles: strips end on a tile edge
    130,     # 5 tiles: the ring wraps; S = 4 leaves a second strip of one tile
    256,     # 8 tiles: exactly one strip at S = 8
    257,     # 9 tiles: S = 8 leaves a second strip of one tile whose left halo comes from memory
    289)     # 10 tiles: S = 3 gives strips 3, 3, 3, 1 and S = 4 gives 4, 4, 2
    for C in (24, 264) for K in (
    7,       # restages from t0 + 14 and leaves stale slots in the ring
    31)]
# the weight-gradient fold: B cdiv(T, 32) partial rows on either side of the 1024 at which the fused entry's fold runs four slices
REDUCE = [("reduce", B, T, 8, K, "randn") for B, T in ((33, 992), (32, 1024)) for K in (7, 31)]      # 1023 and 1024 tiles
OPTIONS = [("options", 2, 70, 264, 15, "randn"), ("options", 2, 33, 12, 31, "randn")]      # bias / dbias None, accumulate 0 | 1


def rule_S(B, T, C, cus):
    """the library's rule under conv_strip = 0: the smallest S <= 8 with B cdiv(cdiv(T, 32), S) cdiv(C, 256) <= 2 CUs"""
    S = 1
    while S < 8 and B * cdiv(cdiv(T, 32), S) * cdiv(C, 256) > 2 * cus:
        S += 1
    return S


def rule_cases(cus):
    """C = 8 (one channel block), B from the device's CU count: T = 289 (10 tiles) with the smallest B at which the rule leaves S = 1
    (it picks S = 2: 5 strips), T = 512 (16 tiles) with the smallest B at which S = 7 (3 strips) is still too many: S = 8"""
    cases = [("rule", 2 * cus // 10 + 1, 289, 8, 31, "randn"), ("rule", 2 * cus // 3 + 1, 512, 8, 7, "randn")]
    assert rule_S(*cases[0][1:4], cus) >= 2 and rule_S(*cases[1][1:4], cus) == 8
    return cases


DW_ALL = TAPS + TIME31 + TIME7 + CHAN_ALL + BATCH           # every path: f32, bf16 plain, bf16 LDS, fused
DW_CASES = DW_ALL + CHAN_PLAIN                               # CHAN_PLAIN: f32 and bf16 on the plain kernel
CHAIN_CASES = DW_ALL + STRIPS

# ("glu", M, C, kind) | ("glum", B, T, C, lens)
GLU_CASES = ([("glu", M, C, "randn") for M in (1, 301) for C in (1, 8, 12, 256, 264)]
             + [("glu", 301, C, "hard") for C in (12, 264)])
GLU_MASKED_CASES = [("glum", 4, 9, C, (0, 1, 8, 9)) for C in (12, 264)] + [("glum", 4, 1, 8, (0, 1, 0, 1))]      # lens 0, 1, T - 1, T
GLU_GATES = (20.0, -20.0, 90.0, -90.0)
GLU_GATES_F32 = (104.0, -104.0)


def case_id(case):
    return "-".join(str(v).replace(" ", "") for v in case)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def conv_inputs(case, dtype):
    """x, dy [B, T, C] and g [B, T, 2C], ds [B, T, C] (the chain's GLU input and the gradient w.r.t. the Swish output) rounded to
    `dtype`; w [C, K], bias, gamma, beta float32; dw0 / db0: the non-zero values dw / db start from"""
    _, B, T, C, K, kind = case
    gen = _gen(case, str(dtype))
    rn = lambda *s: torch.randn(*s, generator=gen)
    x, dy, g, ds = rn(B, T, C), rn(B, T, C), rn(B, T, 2 * C), rn(B, T, C)
    if kind == "edges":
        for t in (x, dy, g[..., :C]):
            t[:, 0] = 64 * torch.sign(t[:, 0])
            t[:, -1] = 64 * torch.sign(t[:, -1])
    return SimpleNamespace(case=case, dtype=dtype, B=B, T=T, C=C, K=K, x=_rt(x, dtype), dy=_rt(dy, dtype), g=_rt(g, dtype),
                           ds=_rt(ds, dtype), w=rn(C, K) * K ** -0.5, bias=rn(C), gamma=1 + 0.1 * rn(C), beta=0.1 * rn(C),
                           dw0=rn(C, K), db0=rn(C))


def operands(x, dy, K, dtype):
    """an input set around tensors handed in (the chain's intermediates): what eval_bwd_w / check_bwd_w need"""
    B, T, C = x.shape
    return SimpleNamespace(case=None, dtype=dtype, B=B, T=T, C=C, K=K, x=x, dy=dy, dw0=torch.zeros(C, K), db0=torch.zeros(C))


def glu_inputs(case, dtype):
    """g [M, 2C] (masked: [B, T, 2C]) and d [M, C] rounded to `dtype`.  hard: the gate cycles through +-20, +-90 (and +-104 in f32:
    exp overflows float32 there) and a random value, `a` through 0, +-1e4 and a random value, every combination"""
    gen = _gen(case, str(dtype))
    rn = lambda *s: torch.randn(*s, generator=gen)
    if case[0] == "glum":
        _, B, T, C, lens = case
        return SimpleNamespace(case=case, dtype=dtype, g=_rt(rn(B, T, 2 * C), dtype), lens=torch.tensor(lens, dtype=torch.int32))
    _, M, C, kind = case
    g, d = rn(M, 2 * C), rn(M, C)
    if kind == "hard":
        gates = GLU_GATES + (GLU_GATES_F32 if dtype == F32 else ())
        i = torch.arange(M * C).reshape(M, C)
        gi, ai = i % (len(gates) + 1), (i // (len(gates) + 1)) % 4
        for k, v in enumerate(gates):
            g[:, C:][gi == k] = v
        for k, v in enumerate((0.0, 1e4, -1e4)):
            g[:, :C][ai == k] = v
    return SimpleNamespace(case=case, dtype=dtype, g=_rt(g, dtype), d=_rt(d, dtype))


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


def eval_fwd(inp, dt, bias=True, tap=_no_tap, x=None):
    """x: the input when it is not inp.x (the chain's GLU output)"""
    fn = lambda: dwconv_fwd(*_to(dt, inp.x if x is None else x, inp.w, inp.bias if bias else None), tap=tap)
    return fn() if x is not None else _memo(inp, ("fwd", dt, bias), tap, fn)


def eval_bwd_x(inp, dt, tap=_no_tap, dy=None):
    fn = lambda: dwconv_bwd_x(*_to(dt, inp.dy if dy is None else dy, inp.w), tap=tap, bias=inp.bias.to(dt))
    return fn() if dy is not None else _memo(inp, ("bwd_x", dt), tap, fn)


def eval_bwd_w(inp, dt, tap=_no_tap):
    return _memo(inp, ("bwd_w", dt), tap, lambda: dwconv_bwd_w(*_to(dt, inp.dy, inp.x), inp.K, tap=tap))


def model_fwd(inp, mutant=None, bias=True):
    return _out(eval_fwd(inp, F32, bias, MUTANTS[mutant]), inp.dtype)


def model_bwd_x(inp, mutant=None):
    return _out(eval_bwd_x(inp, F32, MUTANTS[mutant]), inp.dtype)


def model_bwd_w(inp, mutant=None, accumulate=True):
    """dw / db after the accumulation into dw0 / db0 (accumulate = False: from zero)"""
    tap = MUTANTS[mutant]
    dw, db, _, _ = eval_bwd_w(inp, F32, tap)
    return (_acc(tap, inp.dw0, dw), _acc(tap, inp.db0, db)) if accumulate else (dw, db)


def check_fwd(inp, y, bias=True, x=None):
    """y (a CPU tensor) against the float64 reference -> worst share of the bound"""
    ref, m32 = eval_fwd(inp, F64, bias, x=x), eval_fwd(inp, F32, bias, x=x)
    return {"y": share(y, ref, elem_bound(ref, m32, inp.dtype == BF))}


def check_bwd_x(inp, dx, dy=None):
    ref, m32 = eval_bwd_x(inp, F64, dy=dy), eval_bwd_x(inp, F32, dy=dy)
    return {"dx": share(dx, ref, elem_bound(ref, m32, inp.dtype == BF))}


def check_bwd_w(inp, dw=None, db=None, accumulate=True):
    """dw / db: the buffers after the call, which started from inp.dw0 / inp.db0 (accumulate = False: the call stores the sums)"""
    ref, m32 = eval_bwd_w(inp, F64), eval_bwd_w(inp, F32)
    res = {}
    for name, got, k, start in (("dw", dw, 0, inp.dw0), ("db", db, 1, inp.db0)):
        if got is not None:
            r, m = (start.double() + ref[k], start + m32[k]) if accumulate else (ref[k], m32[k])
            res[name] = share(got, r, colsum_bound(r, m, inp.B * inp.T, ref[k + 2]))
    return res


def eval_glu(inp, dt, op, tap=_no_tap):
    def fn():
        if op == "fwd":
            return glu_fwd(inp.g.to(dt), tap)
        if op == "masked":
            return glu_fwd_masked(inp.g.to(dt), inp.lens, tap)
        return glu_bwd(inp.g.to(dt), inp.d.to(dt), tap)
    return _memo(inp, ("glu", op, dt), tap, fn)


def model_glu(inp, op, mutant=None):
    return _out(eval_glu(inp, F32, op, MUTANTS[mutant]), inp.dtype)


def check_glu(inp, op, got):
    ref, m32 = eval_glu(inp, F64, op), eval_glu(inp, F32, op)
    return {{"fwd": "out", "masked": "out", "bwd": "din"}[op]: share(got, ref, elem_bound(ref, m32, inp.dtype == BF))}
