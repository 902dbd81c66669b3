"""The LSTM recurrences restated in plain torch on the CPU (gate order i | f | g | o, z = pre + h_prev . W_hh^T, as torch.nn.LSTM):
the cell and its backward, the unidirectional sequence (csrc/lstm_coop.hip: lstm_seq_*, csrc/rnnt.hip: lstm_cell_*) and the
bidirectional, length-aware layer with the frame map of csrc/bilstm.hip (step s works on frame s forward, len - 1 - s reverse; a row
with s >= len is inactive and leaves zeros at frame s; hprev is the h the cell started from).

Every function takes a dtype (float64: the reference; float32: a model of the kernels' arithmetic) and the places where the kernels
round: `round_to` (stored h, activated gates, gate gradients; c and dc stay in the working precision), `sum_to` (lstm_seq and the
bf16 chain round pre + rec), `rec_to` (bilstm_seq and the bidirectional chain round rec only).  `forced` makes a run ONE-STEP
(teacher-forced): the state every step starts from is taken from the given hseq / cseq (or, backward, the given gate gradients)
instead of the run's own, so rounding cannot accumulate along the sequence.  The mutants of the model (MUTANTS: one indexing /
formula error each; tests/test_lstm_ref_cpu.py shows that the bounds below reject every one) stay out of these functions: they come
in through `tap` / `cell`.

check_uni / check_bi hold a set of outputs -- a kernel's, or the float32 model's -- against the float64 one-step reference and
return the worst share of the bound per tensor; the case tables of the GPU sweep live here too, shared by both test files.
tests/test_lstm_ref_cpu.py pins all of this against torch.nn.LSTM and autograd without a GPU."""
from types import SimpleNamespace

import torch

P8 = 2.0 ** -8          # bf16's worst relative rounding error
BF = torch.bfloat16
F64, F32 = torch.float64, torch.float32


def _rnd(x, to):
    return x if to is None else x.to(to).to(x.dtype)


def _act(z):
    i, f, g, o = z.chunk(4, -1)
    return torch.cat((torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)), -1)


def cell_fwd(z, c_prev):
    """z [..., 4H] -> (activated gates [..., 4H], c, h)"""
    gates = _act(z)
    i, f, g, o = gates.chunk(4, -1)
    c = f * c_prev + i * g
    return gates, c, o * torch.tanh(c)


def cell_bwd(dh, dc, gates, c_prev, c):
    """dh, dc: gradients w.r.t. this cell's h and c -> (dz [..., 4H], dc_prev)"""
    i, f, g, o = gates.chunk(4, -1)
    tc = torch.tanh(c)
    dct = dc + dh * o * (1 - tc * tc)
    dz = torch.cat((dct * g * i * (1 - i), dct * c_prev * f * (1 - f), dct * i * (1 - g * g), dh * tc * o * (1 - o)), -1)
    return dz, dct * f


def _no_tap(point, v, **ctx):
    """the sequence functions pass every operand a kernel has to ADDRESS through tap(point, value, **context) before using it; the
    reference and the model leave them alone, a mutant (MUTANTS below) returns another value at its point"""
    return v


# ---- unidirectional ---------------------------------------------------------------------------------------------------------------
def seq_fwd(pre, w_hh, h0=None, c0=None, dtype=F64, round_to=None, sum_to=None, forced=None, tap=_no_tap, cell=cell_fwd):
    """pre [U,B,4H] -> namespace of [U,B,.] tensors: z, rec, gates, c, h (unrounded), c_prev, and the stored hseq, cseq, gact"""
    U, B, H4 = pre.shape
    H = H4 // 4
    pre, w = pre.to(dtype), w_hh.to(dtype)
    zero = torch.zeros(B, H, dtype=dtype)
    h = zero if h0 is None else h0.to(dtype)
    c = tap("c0", zero if c0 is None else c0.to(dtype))
    keys = "z rec gates c h c_prev hseq cseq gact".split()
    out = {k: [] for k in keys}
    for u in range(U):
        rec = tap("rec", tap("h_prev", h) @ w.t())
        z = _rnd(pre[u] + rec, sum_to)
        gates, cn, hn = cell(z, tap("c_prev", c, s=u))
        for k, v in zip(keys, (z, rec, gates, cn, hn, c, _rnd(hn, round_to), cn, _rnd(gates, round_to))):
            out[k].append(v)
        h, c = (_rnd(hn, round_to), cn) if forced is None else (forced[0][u].to(dtype), forced[1][u].to(dtype))
    return SimpleNamespace(**{k: torch.stack(v) for k, v in out.items()})


def seq_bwd(dh_seq, gact, cseq, c0, w_hh, dtype=F64, round_to=None, forced=None, tap=_no_tap):
    """dh_seq [U,B,H]: gradient w.r.t. the outputs -> dgp [U,B,4H], w.r.t. the gate pre-activations (forced: the given dgp[u + 1]
    is the operand of the recurrent term, dc is carried here)"""
    U, B, H = dh_seq.shape
    dh_seq, gact, cseq, w = dh_seq.to(dtype), gact.to(dtype), cseq.to(dtype), w_hh.to(dtype)
    zero = torch.zeros(B, H, dtype=dtype)
    dc, nxt, dgp = zero, None, [None] * U
    for u in reversed(range(U)):
        dh = dh_seq[u]
        if nxt is not None:
            dh = dh + tap("dgates", nxt) @ w
        cp = cseq[u - 1] if u > 0 else tap("c0", zero if c0 is None else c0.to(dtype))
        dz, dc = cell_bwd(dh, dc, gact[u], cp, cseq[u])
        dgp[u] = _rnd(dz, round_to)
        nxt = dgp[u] if forced is None else forced[u].to(dtype)
    return torch.stack(dgp)


def layer_bwd(dgp, x, hseq, h0, w_ih):
    """the layer's gradients from dgp [U,B,4H]: (g_w_ih, g_w_hh -- its h0 term included --, bias column sums, dx)"""
    U, B, H4 = dgp.shape
    d2 = dgp.reshape(U * B, H4)
    g_w_hh = dgp[1:].reshape(-1, H4).t() @ hseq[:-1].reshape(-1, H4 // 4)
    if h0 is not None:
        g_w_hh = g_w_hh + dgp[0].t() @ h0
    return d2.t() @ x.reshape(U * B, -1), g_w_hh, d2.sum(0), (d2 @ w_ih).view(U, B, -1)


# ---- bidirectional, length-aware --------------------------------------------------------------------------------------------------
def frame_map(lens, T, s):
    """-> (active [B], frame [2,B]) of step s: frame s forward, len - 1 - s reverse; inactive rows (s >= len): frame s"""
    lens = lens.clamp(max=T)
    act = s < lens
    return act, torch.stack((torch.full_like(lens, s), torch.where(act, lens - 1 - s, torch.full_like(lens, s))))


def frames(lens, T):
    """[B,T] bool: the frames inside each utterance"""
    return torch.arange(T)[None, :] < lens.clamp(max=T)[:, None]


def bi_fwd(pre, w_hh, lens, dtype=F64, round_to=None, rec_to=None, forced=None, rec_given=None, tap=_no_tap, cell=cell_fwd):
    """pre [B,T,8H] (direction d's gates at columns 4H d ..), w_hh: the two directions' [4H,H], lens [B] (long) -> namespace of
    [2,B,T,.] tensors: z, rec, gates, c, h, c_prev (unrounded, zeros at padded frames) and the stored hseq, hprev, cseq, gact;
    rec_given[s] [2,B,4H]: the recurrent products handed in (the cell kernels alone)"""
    B, T, H8 = pre.shape
    H = H8 // 8
    pre, w = pre.to(dtype), [x.to(dtype) for x in w_hh]
    ar = torch.arange(B)
    keys = "z rec gates c h c_prev hseq hprev cseq gact".split()
    out = {k: torch.zeros(2, B, T, 4 * H if k in ("z", "rec", "gates", "gact") else H, dtype=dtype) for k in keys}
    h = [torch.zeros(B, H, dtype=dtype) for _ in range(2)]
    c = [torch.zeros(B, H, dtype=dtype) for _ in range(2)]
    for s in range(T):
        act, fr = frame_map(lens, T, s)
        m = act[:, None]
        for d in range(2):
            p = pre[ar, tap("frame", fr[d], d=d, act=act, lens=lens.clamp(max=T)), 4 * H * d:4 * H * (d + 1)]
            if rec_given is not None:
                rec = torch.zeros_like(p) if rec_given[s] is None else rec_given[s][d].to(dtype)
            else:
                rec = _rnd(tap("h_prev", h[d]) @ w[d].t(), rec_to)
            z = p + rec
            gates, cn, hn = cell(z, tap("c_prev", c[d], s=s))
            for k, v in zip(keys, (z, rec, gates, cn, hn, c[d], _rnd(hn, round_to), h[d], cn, _rnd(gates, round_to))):
                out[k][d, ar, fr[d]] = torch.where(m, v, torch.zeros_like(v))
            if forced is None:
                hn_, cn_ = _rnd(hn, round_to), cn
            else:
                hn_, cn_ = forced[0][d, ar, fr[d]].to(dtype), forced[1][d, ar, fr[d]].to(dtype)
            h[d], c[d] = torch.where(m, hn_, torch.zeros_like(hn_)), torch.where(m, cn_, torch.zeros_like(cn_))
    return SimpleNamespace(**out)


def bi_bwd(dy, gact, cseq, w_hh, lens, dtype=F64, round_to=None, rec_to=None, forced=None, rec_given=None, tap=_no_tap):
    """dy [B,T,H]: gradient w.r.t. the masked sum of the two directions -> dg [2,B,T,4H] (exact zeros at padded frames)"""
    B, T, H = dy.shape
    dy, gact, cseq, w = dy.to(dtype), gact.to(dtype), cseq.to(dtype), [x.to(dtype) for x in w_hh]
    ar = torch.arange(B)
    dg = torch.zeros(2, B, T, 4 * H, dtype=dtype)
    dc = [torch.zeros(B, H, dtype=dtype) for _ in range(2)]
    dgc = [torch.zeros(B, 4 * H, dtype=dtype) for _ in range(2)]
    for s in reversed(range(T)):
        act, fr = frame_map(lens, T, s)
        m = act[:, None]
        frp = frame_map(lens, T, s - 1)[1] if s > 0 else None
        for d in range(2):
            dh = dy[ar, fr[d]]
            if s < T - 1:
                dh = dh + (rec_given[s][d].to(dtype) if rec_given is not None else _rnd(tap("dgates", dgc[d]) @ w[d], rec_to))
            # the cell state this one started from: the previous step's frame, zero at the direction's first frame
            cp = cseq[d, ar, frp[d]] if s > 0 else tap("c_first", torch.zeros(B, H, dtype=dtype), cseq=cseq[d], fr=fr[d], d=d)
            dz, dcp = cell_bwd(dh, dc[d], gact[d, ar, fr[d]], cp, cseq[d, ar, fr[d]])
            dzs = torch.where(m, _rnd(dz, round_to), torch.zeros_like(dz))
            dg[d, ar, fr[d]] = dzs
            dgc[d] = dzs if forced is None else torch.where(m, forced[d, ar, fr[d]].to(dtype), torch.zeros_like(dz))
            dc[d] = torch.where(m, dcp, torch.zeros_like(dcp))
    return dg


def bi_hprev_of(hseq, lens):
    """the hprev a correct layer stores beside hseq [2,B,T,H]: the neighbouring frame's h, zeros at each direction's first frame and
    at padded frames"""
    T = hseq.shape[2]
    hp = torch.zeros_like(hseq)
    hp[0, :, 1:] = hseq[0, :, :-1]
    hp[1, :, :-1] = hseq[1, :, 1:]
    return hp * frames(lens, T)[None, :, :, None].to(hseq.dtype)


# ---- bounds (none taken from the code under test; derivation: tests/test_lstm_kernels_gpu.py) --------------------------------------
def _e32(m32, ref):
    return float((m32.double() - ref).abs().max()) if ref.numel() else 0.0


def fwd_bounds(ref, m32, bf16, z_rounded):
    """bounds of the stored gates, c and h around the float64 one-step reference `ref`; m32: the float32 evaluation of the same
    step; z_rounded: the kernel rounds rec or pre + rec to bf16 (else z is taken as exact: the cell kernels given their operands)"""
    e = {k: _e32(getattr(m32, k), getattr(ref, k)) for k in ("z", "gates", "c", "h")}
    if not bf16:
        return {k: torch.full_like(getattr(ref, k), max(4 * e[k], 1e-5 * float(getattr(ref, k).abs().max()))) for k in ("gates", "c", "h")}
    a = ref.gates
    b_a = torch.full_like(a, max(4 * e["gates"], 1e-6))
    if z_rounded:
        dz = P8 * torch.maximum(ref.z.abs(), ref.rec.abs()) + 4 * e["z"]
        b_a = b_a + torch.maximum((_act(ref.z + dz) - a).abs(), (_act(ref.z - dz) - a).abs())
    b_i, b_f, b_g, b_o = b_a.chunk(4, -1)
    i, f, g, o = a.abs().chunk(4, -1)
    b_c = ref.c_prev.abs() * b_f + g * b_i + i * b_g + b_i * b_g + torch.clamp(1e-6 * (1 + ref.c.abs()), min=4 * e["c"])
    b_h = b_o + o * b_c + b_o * b_c + P8 * ref.h.abs() + max(4 * e["h"], 1e-6)
    return {"gates": b_a + P8 * a.abs(), "c": b_c, "h": b_h}


def bwd_bound(ref, m32, bf16):
    e = _e32(m32, ref)
    if not bf16:
        return torch.full_like(ref, max(4 * e, 1e-5 * float(ref.abs().max())))
    return P8 * ref.abs() + max(4 * e, 1e-7)


def share(got, ref, bound, sel=None):
    """worst |got - ref| / bound over the selected entries (every selected entry of got must be finite)"""
    got = got.double()
    if sel is not None:
        sel = sel.expand_as(ref)
        got, ref, bound = got[sel], ref[sel], bound[sel]
    if ref.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), "non-finite value where the operation defines one"
    return float(((got - ref).abs() / bound).max())


def check_uni(inp, hseq, cseq, gact, dgp, bf16=True, z_rounded=True):
    """a unidirectional layer's outputs (CPU tensors) against the one-step float64 reference -> worst share of the bound per tensor.
    The backward is checked on the given gact / cseq, as the kernel ran on them."""
    forced = (hseq, cseq)
    ref = seq_fwd(inp.pre, inp.w_hh, inp.h0, inp.c0, forced=forced)
    m32 = seq_fwd(inp.pre, inp.w_hh, inp.h0, inp.c0, dtype=F32, forced=forced)
    b = fwd_bounds(ref, m32, bf16, z_rounded)
    res = {"gact": share(gact, ref.gates, b["gates"]), "c": share(cseq, ref.c, b["c"]), "h": share(hseq, ref.h, b["h"])}
    if dgp is not None:
        rb = seq_bwd(inp.dh, gact, cseq, inp.c0, inp.w_hh, forced=dgp)
        mb = seq_bwd(inp.dh, gact, cseq, inp.c0, inp.w_hh, dtype=F32, forced=dgp)
        res["dgp"] = share(dgp, rb, bwd_bound(rb, mb, bf16))
    return res


def check_bi(inp, hseq, hprev, cseq, gact, dg, bf16=True, z_rounded=True, rec_given=None, drec_given=None, rec_to=None):
    """the bidirectional layer's outputs likewise; exact: zeros at padded frames, hprev = the neighbouring hseq bit for bit and zero
    at each direction's first frame"""
    T = hseq.shape[2]
    fm = frames(inp.lens, T)[None, :, :, None]
    for name, t in (("hseq", hseq), ("hprev", hprev), ("cseq", cseq), ("gact", gact)) + ((("dg", dg),) if dg is not None else ()):
        pad = t[(~fm).expand_as(t)]
        assert bool((pad == 0).all()), f"{name}: a padded frame is not exact zeros"
    assert torch.equal(hprev.double(), bi_hprev_of(hseq.double(), inp.lens)), "hprev is not the neighbouring frame's hseq"
    forced = (hseq, cseq)
    kw = dict(forced=forced, rec_given=rec_given, rec_to=rec_to)
    ref = bi_fwd(inp.pre, inp.w_hh, inp.lens, **kw)
    m32 = bi_fwd(inp.pre, inp.w_hh, inp.lens, dtype=F32, **kw)
    b = fwd_bounds(ref, m32, bf16, z_rounded)
    res = {"gact": share(gact, ref.gates, b["gates"], fm), "c": share(cseq, ref.c, b["c"], fm), "h": share(hseq, ref.h, b["h"], fm)}
    if dg is not None:
        kw = dict(forced=dg, rec_given=drec_given, rec_to=rec_to)
        rb = bi_bwd(inp.dy, gact, cseq, inp.w_hh, inp.lens, **kw)
        mb = bi_bwd(inp.dy, gact, cseq, inp.w_hh, inp.lens, dtype=F32, **kw)
        res["dg"] = share(dg, rb, bwd_bound(rb, mb, bf16), fm)
    return res


# ---- the float32 model of the cooperative kernels (their documented roundings), and its mutants --------------------------------------
def _at(points, fn):
    """a tap that replaces the value at these points by fn(value, **context)"""
    return lambda point, v, **ctx: fn(v, **ctx) if point in points else v


def _drop_slice(rec, **ctx):
    rec = rec.clone()
    rec.view(rec.shape[0], 4, -1)[:, :, 16:32] = 0
    return rec


def _row_minus_32(c, **ctx):
    out = c.clone()
    for m0 in range(0, c.shape[0], 64):
        n = min(c.shape[0], m0 + 64) - (m0 + 32)
        if n > 0:
            out[m0 + 32:m0 + 32 + n] = c[m0:m0 + n]
    return out


def _drop_tail(d, **ctx):
    H = d.shape[-1] // 4
    G = H // 16
    d = d.clone()
    d.view(d.shape[0], 4, H)[..., 16 * (G - G % 8):] = 0
    return d


def _rev_frame(off):
    def fn(fr, d, act, lens, **ctx):
        return torch.where(act & (d == 1), (fr + off).clamp(min=0).minimum(lens - 1), fr)
    return fn


def _stale_c(point, v, **ctx):
    if point == "c_prev" and ctx["s"] == 0:        # forward: whatever the register held
        return torch.full_like(v, 0.5)
    if point == "c_first":                         # backward: the neighbouring frame in memory
        B, T, H = ctx["cseq"].shape
        return ctx["cseq"].reshape(B * T, H).roll(1 if ctx["d"] == 0 else -1, 0).view(B, T, H)[torch.arange(B), ctx["fr"]]
    return v


def _cell_if_swapped(z, c_prev):
    gates, _, _ = cell_fwd(z, c_prev)
    i, f, g, o = gates.chunk(4, -1)
    c = i * c_prev + f * g
    return gates, c, o * torch.tanh(c)


# one indexing / formula error each, as keyword arguments of the sequence functions above
MUTANTS = {
    None: {},
    "swap_if": dict(cell=_cell_if_swapped),                               # i and f gates swapped
    "row_plus1": dict(tap=_at({"h_prev"}, lambda h, **ctx: h.roll(-1, 0))),   # h_prev taken from row b + 1
    "rev_plus1": dict(tap=_at({"frame"}, _rev_frame(1))),                 # reverse direction on frame len - s - 1 + 1
    "rev_minus1": dict(tap=_at({"frame"}, _rev_frame(-1))),               # ... - 1
    "c_first": dict(tap=_stale_c),                                        # c_prev not zeroed at a direction's first frame
    "c0_ignored": dict(tap=_at({"c0"}, lambda c, **ctx: torch.zeros_like(c))),
    "slice_drop": dict(tap=_at({"rec"}, _drop_slice)),                    # the recurrent term of units 16 .. 31 dropped
    "row32": dict(tap=_at({"c_prev"}, _row_minus_32)),                    # rows >= 32 of a 64-row group on row m - 32's cell state
    "partial_tail": dict(tap=_at({"dgates"}, _drop_tail)),                # the last G % 8 workgroups' partials left out (G = H / 16)
}


def model_uni(inp, mutant_fwd=None, mutant_bwd=None):
    """lstm_seq_fwd + lstm_seq_bwd: pre + rec rounded to bf16, h / gact / dgp stored in bf16, c and dc f32, dh formed in f32"""
    f = seq_fwd(inp.pre, inp.w_hh, inp.h0, inp.c0, dtype=F32, round_to=BF, sum_to=BF, **MUTANTS[mutant_fwd])
    dgp = seq_bwd(inp.dh, f.gact, f.cseq, inp.c0, inp.w_hh, dtype=F32, round_to=BF, **MUTANTS[mutant_bwd])
    return f.hseq, f.cseq, f.gact, dgp


def model_bi(inp, mutant_fwd=None, mutant_bwd=None):
    """bilstm_seq_fwd + bilstm_seq_bwd: rec rounded to bf16, the rest as model_uni"""
    f = bi_fwd(inp.pre, inp.w_hh, inp.lens, dtype=F32, round_to=BF, rec_to=BF, **MUTANTS[mutant_fwd])
    dg = bi_bwd(inp.dy, f.gact, f.cseq, inp.w_hh, inp.lens, dtype=F32, round_to=BF, **MUTANTS[mutant_bwd])
    return f.hseq, f.hprev, f.cseq, f.gact, dg


# ---- the cases of the sweep -------------------------------------------------------------------------------------------------------
# unidirectional cooperative: (family, U, B, H, state) with state in "both" | "none" | "h0" | "c0"; family "hard": pre entries of
# +-60 and |c0| ~ 5, so that the cell state reaches |c| ~ 6
UNI_CASES = ([("rows", 3, B, 64, "both") for B in (1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 128, 129)]
             + [("groups", 4, 512, 128, "both")]
             + [("hidden", 3, 17, H, "both") for H in (32, 96, 160, 288, 512)]
             + [("height", 3, 150, 512, "both")]
             + [("length", U, 17, 64, "both") for U in (2, 6)]
             + [("state", 3, 17, 64, s) for s in ("none", "h0", "c0")]
             + [("hard", 3, 17, 64, "both"), ("hard", 3, 33, 160, "both")])
# bidirectional cooperative: (family, B, T, H, length pattern, pad columns of pre's rows); patterns: "full" all T, "ones" all 1,
# "mixed" T, 1, T - 1, 2, ... with the full-length row first and last, "group": a 64-row group of length 1 beside a full one;
# family "hard": pre entries of +-60, and four units per direction whose cell state reaches |c| = len (7 at T = 7; there is no c0)
BI_CASES = ([("rows", B, 3, 64, "mixed", 0) for B in (1, 16, 17, 33, 64, 65, 129, 256)]
            + [("hidden", 17, 3, H, "mixed", 0) for H in (32, 96, 160, 512)]
            + [("length", 17, T, 64, "mixed", 0) for T in (2, 7)]
            + [("lengths", 17, 3, 64, "full", 0), ("lengths", 17, 3, 64, "ones", 0), ("lengths", 128, 3, 64, "group", 0),
               ("lengths", 33, 7, 96, "mixed", 0)]
            + [("stride", 17, 3, 64, "mixed", 8)]
            + [("hard", 17, 3, 64, "mixed", 0), ("hard", 33, 7, 160, "mixed", 0)])


def case_id(case):
    return "-".join(str(v) for v in case)


def lengths(pattern, B, T):
    if pattern == "full":
        lens = [T] * B
    elif pattern == "ones":
        lens = [1] * B
    elif pattern == "group":
        lens = [1 if b < 64 else T for b in range(B)]
    else:
        lens = [(T - b // 2) if b % 2 == 0 else (1 + b // 2) for b in range(B)]
        lens = [1 + (v - 1) % T for v in lens]
        lens[0] = lens[-1] = T
    return torch.tensor(lens, dtype=torch.long)


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum(int(v) * p for v, p in zip(key, (1000003, 10007, 101, 7))) + 20240)
    return g


def _bf(x):
    return x.to(BF).float()


def _hard(pre, g):
    """a quarter of the entries at +-60 (exp overflows to inf in the hardware forms of tanh)"""
    hit = torch.rand(pre.shape, generator=g) < 0.25
    sign = torch.where(torch.rand(pre.shape, generator=g) < 0.5, -1.0, 1.0)
    return torch.where(hit, 60.0 * sign, pre)


def uni_inputs(case):
    """CPU float32 tensors holding bf16 values (c0: f32): pre scale 1, w_hh scale H^-0.5, h0 / c0 scale 0.5, dh scale 0.5"""
    family, U, B, H, state = case
    g = _gen(U, B, H, len(state) + 10 * (family == "hard"))
    rn = lambda *s: torch.randn(*s, generator=g)
    pre, w_hh, dh = _bf(rn(U, B, 4 * H)), _bf(rn(4 * H, H) * H ** -0.5), _bf(rn(U, B, H) * 0.5)
    h0 = _bf(rn(B, H) * 0.5) if state in ("both", "h0") else None
    c0 = rn(B, H) * 0.5 if state in ("both", "c0") else None
    if family == "hard":
        pre = _hard(pre, g)
        c0 = torch.where(c0 < 0, -5.0, 5.0) + c0
    return SimpleNamespace(pre=pre, w_hh=w_hh, h0=h0, c0=c0, dh=dh)


def bi_inputs(case):
    family, B, T, H, pattern, pad = case
    g = _gen(B, T, H, len(pattern) + 10 * (family == "hard"))
    rn = lambda *s: torch.randn(*s, generator=g)
    pre = _bf(rn(B, T, 8 * H))
    w_hh = [_bf(rn(4 * H, H) * H ** -0.5) for _ in range(2)]
    dy = _bf(rn(B, T, H) * 0.5)
    if family == "hard":
        pre = _hard(pre, g)
        for d in range(2):      # units 0 .. 3: i, f at +60 and g at +-60 on every frame, so that |c| grows by 1 per step, to len
            for j in range(4):
                col = 4 * H * d + j
                pre[:, :, col] = pre[:, :, col + H] = 60.0
                pre[:, :, col + 2 * H] = 60.0 if j % 2 == 0 else -60.0
    return SimpleNamespace(pre=pre, w_hh=w_hh, lens=lengths(pattern, B, T), dy=dy)
