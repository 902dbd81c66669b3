"""The LSTM recurrence kernels against the float64 restatement of tests/lstm_ref.py (pinned on the CPU by tests/test_lstm_ref_cpu.py):
the cooperative whole-sequence kernels of csrc/lstm_coop.hip (lstm_seq_fwd / bwd, bilstm_seq_fwd / bwd), the cell kernels of
csrc/rnnt.hip (lstm_cell_fwd / bwd) and csrc/bilstm.hip (bilstm_cell_fwd / bwd, bilstm_out), and recurrence.lstm_layer_fwd / bwd,
at the edges where the kernels change path: B on both sides of the 16-row MFMA tiles (16 * mt < B, row tiles split between waves
0-3 and 4-7, the second (row, unit) pair of a thread from row 32), a second barrier group of one row (B 65) and eight groups, H = 32
(G = 2, one k step, two waves with a column strip in the backward), G % 8 != 0 (the partial trip of the backward's sum over the
workgroups' partials), U = 2 (one barrier) and 3 (both halves of the partial double buffer), h0 without c0 and c0 without h0, a
pre row stride above 8H, every length pattern of the bidirectional frame map.

All checks are ONE-STEP (teacher-forced): step u is evaluated in float64 from the kernel's OWN h_{u-1} / c_{u-1} (the frame the
operation defines; h0 / c0 or zeros at the first) and the same bf16-rounded inputs, the backward's recurrent term from the kernel's
own stored dgp[u + 1] (exactly the operands the kernel multiplies; dc is carried in the reference).  Rounding error then cannot
accumulate along the sequence and the bounds are derived, not tuned; by induction over u they pin the whole recurrence: a stale or
misaddressed h_{u-1} -- a barrier race, a read across groups -- fails at step u.

Bounds (tests/lstm_ref.py: fwd_bounds, bwd_bound; none taken from the kernels).  P8 = 2^-8: bf16's worst relative rounding error.
e32: the error of the float32 evaluation of the same step without roundings on the same case; the factor 4 and the 1e-6 floor as in
tests/test_ctc_loss_gpu.py: the hardware exp / rcp forms (a few ulp; common.h: tanh_fast ~1e-7 absolute, the v_rcp sigmoid 1 ulp)
and another summation order.
  gates (bf16 cooperative)  rec = h_{u-1} . W_hh^T, z = pre + rec; the kernel rounds z (lstm_seq) or rec (bilstm_seq) to bf16:
                            dz = P8 max(|z|, |rec|) + 4 e32(z); unrounded gate b_a = max |act(z +- dz) - act(z)| + max(4 e32, 1e-6)
                            (an interval through the monotone activation); stored gate: b_a + P8 |act(z)|
  c                         b_c = |c_prev| b_f + |g| b_i + |i| b_g + b_i b_g + max(4 e32, 1e-6 (1 + |c|))
  h                         b_h = b_o + |o| b_c + b_o b_c + P8 |h| + max(4 e32, 1e-6)      (|tanh'| <= 1)
  dgp                       P8 |ref| + max(4 e32, 1e-7)
  cell kernels, bf16        the same with dz = 0 (the pre-activations / recurrent products are handed in)
  dc of lstm_cell_bwd       max(4 e32, 1e-6 (1 + |dc|)): an f32 quantity like c
  f32 instantiations        max(4 e32, 1e-5 max|ref|): the suite's bar for "the layer alone"
  layer gradients           1e-3 max|ref| against float64 autograd: the suite's bar for f32 / f32x3 products
  padded frames, hprev = the neighbouring hseq, zeros at a direction's first frame, the cell kernels' state buffers, NaN guards,
  refusals, emoasr_lstm_coop_status == 0   exact
Every output buffer is NaN-filled with a NaN guard behind it: after the launch every defined element is finite, the guard untouched.

MEASURED on an MI355X, worst share of the bound per family (the "[measured] lstm <family>" lines this module prints when it is done;
gact | c | h | dgp):
  lstm_seq     rows 0.985 | 0.903 | 0.723 | 0.995    groups 0.988 | 0.946 | 0.804 | 0.995    hidden 0.981 | 0.922 | 0.734 | 0.991
               height 0.994 | 0.938 | 0.755 | 0.993  length 0.963 | 0.846 | 0.662 | 0.990    state 0.988 | 0.905 | 0.731 | 0.993
               hard 0.981 | 0.954 | 0.973 | 0.986
  bilstm_seq   rows 0.992 | 0.879 | 0.794 | 0.994    hidden 0.992 | 0.872 | 0.798 | 0.994    length 0.984 | 0.779 | 0.613 | 0.985
               lengths 0.992 | 0.893 | 0.662 | 0.992 stride 0.976 | 0.692 | 0.722 | 0.990    hard 0.984 | 0.952 | 0.913 | 0.992
  bilstm_cell  f32 0.010 | 0.013 | 0.019 | 0.016     bf16 0.996 | 0.067 | 0.988 | 0.994
  lstm_cell    f32 0.009 | 0.012 | 0.017 | 0.014, dc 0.089          bf16 0.992 | 0.069 | 0.986 | 0.993, dc 0.176
  layer        f32 0.000 on every tensor, f32x3 at most 0.015 (hseq) of the 1e-3 bar
(the shares near 1 are bf16 output rounding, whose worst case 2^-8 IS the bound; in that one run the cooperative kernels' shares
were, case by case, the float32 model's of tests/test_lstm_ref_cpu.py to two digits -- an observation, not something the suite
checks; the f32 kernels sit at the float32 model's error).  The barrier status was zero throughout.

What the sweep exposed: recurrence.lstm_layer_bwd left dgp[0]^T . h0 out of g_w_hh (position 0's gates contain h0 . W_hh^T):
test_layer_gradients_against_float64_autograd[*-h0c0] fails on g_w_hh without it (f32 and f32x3: 951 times the 1e-3 bar, every
other tensor unchanged).  The kernels themselves held every bound."""
from types import SimpleNamespace

import pytest
import torch

from tests import lstm_ref as R

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


def _nan_out(dev, shape, dtype):
    """a NaN-filled tensor of this shape with 64 NaN guard elements behind it -> (tensor, guard)"""
    n = 1
    for v in shape:
        n *= v
    flat = torch.full((n + 64,), NAN, device=dev, dtype=dtype)
    return flat[:n].view(*shape), flat[n:]


def _untouched(*guards):
    return all(bool(torch.isnan(g).all()) for g in guards)


def _status():
    from emoasr_amd import lib
    return lib.size_query("emoasr_lstm_coop_status")


_WORST = {}      # family -> tensor -> worst share of the bound over the family's cases


def _report(family, case, res):
    """every case must be inside its bounds; the worst shares are kept per family and printed once, when the module is done"""
    w = _WORST.setdefault(family, {})
    for k, v in res.items():
        w[k] = max(v, w.get(k, 0.0))
    assert max(res.values()) <= 1.0, (family, case, res)


@pytest.fixture(scope="module", autouse=True)
def _measured():
    yield
    for family, w in _WORST.items():
        print(f"\n[measured] lstm {family}: " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()) + " share of bound", end="")
    print()


def _cpu(t):
    return t.detach().to("cpu", torch.float64 if t.dtype == torch.float64 else F32)


# ---- the cooperative kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.UNI_CASES, ids=R.case_id)
def test_lstm_seq_one_step(dev, case):
    from emoasr_amd import ops
    family, U, B, H, state = case
    inp = R.uni_inputs(case)
    up = lambda t, dt=BF: None if t is None else t.to(dt).to(dev)
    pre, w_hh, h0, c0, dh = up(inp.pre), up(inp.w_hh), up(inp.h0), up(inp.c0, F32), up(inp.dh)
    assert ops.lstm_seq_supported(pre, B, H)
    (hseq, g0), (cseq, g1) = _nan_out(dev, (U, B, H), BF), _nan_out(dev, (U, B, H), F32)
    (gact, g2), (dgp, g3) = _nan_out(dev, (U, B, 4 * H), BF), _nan_out(dev, (U, B, 4 * H), BF)
    ops.lstm_seq_fwd(pre, w_hh, h0, c0, hseq, cseq, gact)
    ops.lstm_seq_bwd(dh, gact, cseq, c0, w_hh, dgp)
    torch.cuda.synchronize()
    assert _status() == 0
    assert _untouched(g0, g1, g2, g3), "a store behind an output"
    if family == "hard":
        assert float(cseq.abs().max()) > 5.5      # (the case is what it claims to be)
    _report(f"lstm_seq {family}", case, R.check_uni(inp, _cpu(hseq), _cpu(cseq), _cpu(gact), _cpu(dgp)))


@pytest.mark.parametrize("case", R.BI_CASES, ids=R.case_id)
def test_bilstm_seq_one_step(dev, case):
    from emoasr_amd import ops
    family, B, T, H, pattern, pad = case
    inp = R.bi_inputs(case)
    ldp = 8 * H + pad
    buf = torch.full((B, T, ldp), NAN, dtype=BF)
    buf[..., :8 * H] = inp.pre.to(BF)      # (the pad columns stay NaN: never read)
    pre = buf.to(dev)[..., :8 * H]
    w_hh = [w.to(BF).to(dev) for w in inp.w_hh]
    dy = inp.dy.to(BF).to(dev)
    elens = inp.lens.to(torch.int32).to(dev)
    assert ops.bilstm_seq_supported(pre, B, H)
    (hseq, g0), (hprev, g1) = _nan_out(dev, (2, B, T, H), BF), _nan_out(dev, (2, B, T, H), BF)
    (cseq, g2), (gact, g3) = _nan_out(dev, (2, B, T, H), F32), _nan_out(dev, (2, B, T, 4 * H), BF)
    dg, g4 = _nan_out(dev, (2, B, T, 4 * H), BF)
    ops.bilstm_seq_fwd(elens, pre, w_hh[0], w_hh[1], hseq, hprev, cseq, gact)
    ops.bilstm_seq_bwd(elens, dy, gact, cseq, w_hh[0], w_hh[1], dg)
    torch.cuda.synchronize()
    assert _status() == 0
    assert _untouched(g0, g1, g2, g3, g4), "a store behind an output"
    for t in (hseq, hprev, cseq, gact, dg):
        assert bool(torch.isfinite(t).all())      # every frame of every row is written, the padded ones included
    if family == "hard":      # (no c0 here: the planted units reach |c| = len on the full-length rows)
        assert float(cseq.abs().max()) > min(T, 6) - 0.5
    _report(f"bilstm_seq {family}", case, R.check_bi(inp, _cpu(hseq), _cpu(hprev), _cpu(cseq), _cpu(gact), _cpu(dg)))


# ---- the cell kernels alone: the recurrent products are formed in float64 on the host and handed in ----------------------------------
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,H", [(5, 7, 24), (70, 3, 64), (3, 4, 1000)])
def test_bilstm_cell_chain_one_step(dev, B, T, H, dtype):
    from emoasr_amd import ops
    ar = torch.arange(B)
    worst = {}
    # the length patterns of the cooperative sweep; "group" (64 rows of length 1 beside full ones) needs more than 64 rows
    for pattern in ("full", "ones", "mixed") + (("group",) if B > 64 else ()):
        inp = R.bi_inputs(("chain", B, T, H, pattern, 0))
        pre, dy = inp.pre.to(dtype).to(dev), inp.dy.to(dtype).to(dev)
        w64 = [w.double() for w in inp.w_hh]
        elens = inp.lens.to(torch.int32).to(dev)
        (hseq, g0), (hprev, g1) = _nan_out(dev, (2, B, T, H), dtype), _nan_out(dev, (2, B, T, H), dtype)
        (cseq, g2), (gact, g3) = _nan_out(dev, (2, B, T, H), F32), _nan_out(dev, (2, B, T, 4 * H), dtype)
        (hstate, g4), (cstate, g5) = _nan_out(dev, (2, B, H), dtype), _nan_out(dev, (2, B, H), F32)
        recs = []
        for s in range(T):
            rec = None
            if s > 0:      # from the kernel's own state, rounded to the dtype: what the product kernels hand over
                hs = hstate.cpu().double()
                rec = torch.stack([hs[d] @ w64[d].t() for d in range(2)]).to(dtype)
            recs.append(None if rec is None else rec.double())
            ops.bilstm_cell_fwd(s, elens, pre, None if rec is None else rec.to(dev), hstate, cstate, hseq, hprev, cseq, gact)
            act, fr = R.frame_map(inp.lens, T, s)
            for d in range(2):     # the state buffers: this step's h / c, zeros for an inactive row
                m = act[:, None].to(dev)
                assert torch.equal(hstate[d], torch.where(m, hseq[d, ar, fr[d]], torch.zeros_like(hstate[d]))), (pattern, s, d)
                assert torch.equal(cstate[d], torch.where(m, cseq[d, ar, fr[d]], torch.zeros_like(cstate[d]))), (pattern, s, d)
        (dg, g6), (dgc, g7) = _nan_out(dev, (2, B, T, 4 * H), dtype), _nan_out(dev, (2, B, 4 * H), dtype)
        dcstate, g8 = _nan_out(dev, (2, B, H), F32)
        drecs = [None] * T
        for s in reversed(range(T)):
            drec = None
            if s < T - 1:
                d64 = dgc.cpu().double()
                drec = torch.stack([d64[d] @ w64[d] for d in range(2)]).to(dtype)
                drecs[s] = drec.double()
            ops.bilstm_cell_bwd(s, elens, dy, None if drec is None else drec.to(dev), dcstate, gact, cseq, dg, dgc)
            act, fr = R.frame_map(inp.lens, T, s)
            for d in range(2):
                assert torch.equal(dgc[d], dg[d, ar, fr[d]]), (pattern, s, d)
        torch.cuda.synchronize()
        assert _untouched(g0, g1, g2, g3, g4, g5, g6, g7, g8), "a store behind an output"
        for t in (hseq, hprev, cseq, gact, dg, hstate, cstate, dgc, dcstate):
            assert bool(torch.isfinite(t).all())
        res = R.check_bi(inp, _cpu(hseq), _cpu(hprev), _cpu(cseq), _cpu(gact), _cpu(dg), bf16=dtype == BF, z_rounded=False,
                         rec_given=recs, drec_given=drecs)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in res.items()}
    _report(f"bilstm_cell {'bf16' if dtype == BF else 'f32'}", (B, T, H), worst)


@pytest.mark.parametrize("with_state", [True, False], ids=["c_prev+dh_rec", "no_state"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H", [(1, 8), (17, 100), (36, 512)])
def test_lstm_cell_one_step(dev, B, H, dtype, with_state):
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + H)
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dtype).float()
    z, dh_out, dh_rec = rn(B, 4 * H, sc=1.5), rn(B, H, sc=0.5), rn(B, H, sc=0.5) if with_state else None
    c_prev = torch.randn(B, H, generator=g) * 0.7 if with_state else None
    dc_in = torch.randn(B, H, generator=g) * 0.3
    up = lambda t, dt=dtype: None if t is None else t.to(dt).to(dev)
    hbuf, g0 = _nan_out(dev, (B, 2 * H), dtype)      # h_out with a row stride of 2H: the pad columns stay NaN
    (c, g1), (gact, g2), (dgp, g3) = _nan_out(dev, (B, H), F32), _nan_out(dev, (B, 4 * H), dtype), _nan_out(dev, (B, 4 * H), dtype)
    ops.lstm_cell_fwd(up(z), up(c_prev, F32), hbuf[:, :H], c, gact)
    dbuf = torch.full((B, 2 * H), NAN, dtype=dtype)
    dbuf[:, :H] = dh_out.to(dtype)
    dbuf = dbuf.to(dev)
    dc = up(dc_in, F32)
    ops.lstm_cell_bwd(dbuf[:, :H], up(dh_rec), dc, gact, up(c_prev, F32), c, dgp)
    torch.cuda.synchronize()
    assert _untouched(g0, g1, g2, g3) and bool(torch.isnan(hbuf[:, H:]).all()), "a store outside the outputs"
    zero = torch.zeros(B, H, dtype=torch.float64)
    cp = zero if c_prev is None else c_prev.double()

    def fwd(dt):
        gates, cn, hn = R.cell_fwd(z.to(dt), cp.to(dt))
        return SimpleNamespace(z=z.to(dt), rec=torch.zeros(B, 4 * H, dtype=dt), gates=gates, c=cn, h=hn, c_prev=cp.to(dt))
    ref, m32 = fwd(torch.float64), fwd(F32)
    b = R.fwd_bounds(ref, m32, dtype == BF, False)
    res = {"gact": R.share(_cpu(gact), ref.gates, b["gates"]), "c": R.share(_cpu(c), ref.c, b["c"]),
           "h": R.share(_cpu(hbuf[:, :H]), ref.h, b["h"])}
    # the backward on the kernel's own gates and c
    dh = dh_out.double() + (0 if dh_rec is None else dh_rec.double())
    bwd = lambda dt: R.cell_bwd(dh.to(dt), dc_in.to(dt), _cpu(gact).to(dt), cp.to(dt), _cpu(c).to(dt))
    (rz, rc), (mz, mc) = bwd(torch.float64), bwd(F32)
    res["dgp"] = R.share(_cpu(dgp), rz, R.bwd_bound(rz, mz, dtype == BF))
    res["dc"] = R.share(_cpu(dc), rc, torch.clamp(1e-6 * (1 + rc.abs()), min=4 * float((mc.double() - rc).abs().max())))
    _report(f"lstm_cell {'bf16' if dtype == BF else 'f32'}", (B, H, with_state), res)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_bilstm_out_sum_mask_and_dropout(dev, dtype):
    from emoasr_amd import ops
    B, T, H = 5, 7, 24
    g = torch.Generator().manual_seed(11)
    x0, x1 = (torch.randn(B, T, H, generator=g).to(dtype).to(dev) for _ in range(2))
    lens = R.lengths("mixed", B, T)
    elens = lens.to(torch.int32).to(dev)
    fm = R.frames(lens, T).to(dev)[:, :, None]
    zero = torch.zeros_like(x0)
    assert torch.equal(ops.bilstm_out(elens, x0, x1), torch.where(fm, (x0.float() + x1.float()).to(dtype), zero))
    assert torch.equal(ops.bilstm_out(elens, x0), torch.where(fm, x0, zero))
    # p = 0.25: the keep pattern of ops.scale_dropout on the flat index, padded frames exact zeros; one rounding of (x0 + x1) / (1 - p)
    p, seed = 0.25, 0x5EED
    keep = ops.scale_dropout(torch.ones(B, T, H, device=dev), 1.0, p, seed) != 0
    assert 0.6 < float(keep.float().mean()) < 0.9
    for second in (x1, None):
        y = ops.bilstm_out(elens, x0, second, p, seed)
        s = x0.double() + (0 if second is None else second.double())
        ref = torch.where(fm & keep, s / (1 - p), torch.zeros_like(s))
        assert bool((y[~(fm & keep).expand_as(y)] == 0).all())
        bound = (R.P8 if dtype == BF else 0.0) * ref.abs() + 1e-6 * ref.abs()      # (f32: a few ulp of the sum and the product)
        assert bool(((y.double() - ref).abs() <= bound).all())


# ---- refusals (exact) -------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from emoasr_amd import lib, ops
    bf, f32 = torch.empty(1, device=dev, dtype=BF), torch.empty(1, device=dev, dtype=F32)
    assert ops.lstm_seq_supported(bf, 512, 64) and ops.lstm_seq_supported(bf, 17, 512) and ops.bilstm_seq_supported(bf, 256, 64)
    assert not ops.lstm_seq_supported(f32, 17, 64)
    assert not ops.lstm_seq_supported(bf, 513, 64)
    assert not ops.lstm_seq_supported(bf, 17, 48)
    assert not ops.lstm_seq_supported(bf, 17, 544)
    assert not ops.bilstm_seq_supported(bf, 257, 64)
    with lib.options(lstm_coop=0):
        assert not ops.lstm_seq_supported(bf, 17, 64) and not ops.bilstm_seq_supported(bf, 17, 64)
    assert ops.lstm_seq_supported(bf, 17, 64)
    # a direct launch at a refused shape raises and writes nothing
    U, B, H = 3, 17, 48
    pre, w_hh = torch.zeros(U, B, 4 * H, device=dev, dtype=BF), torch.zeros(4 * H, H, device=dev, dtype=BF)
    (hseq, g0), (cseq, g1), (gact, g2) = _nan_out(dev, (U, B, H), BF), _nan_out(dev, (U, B, H), F32), _nan_out(dev, (U, B, 4 * H), BF)
    with pytest.raises(lib.EmoasrHipError, match="unsupported shape"):
        ops.lstm_seq_fwd(pre, w_hh, None, None, hseq, cseq, gact)
    torch.cuda.synchronize()
    for t in (hseq, cseq, gact, g0, g1, g2):
        assert bool(torch.isnan(t).all())
    assert _status() == 0


# ---- the layer: recurrence.lstm_layer_fwd / bwd in f32 and f32x3 against float64 autograd --------------------------------------------
@pytest.mark.parametrize("with_state", [False, True], ids=["zero_state", "h0c0"])
@pytest.mark.parametrize("split", [False, True], ids=["f32", "f32x3"])
def test_layer_gradients_against_float64_autograd(dev, split, with_state):
    """the h0c0 cases fail on g_w_hh without the dgp[0]^T . h0 term of recurrence.lstm_layer_bwd"""
    from emoasr_amd import ops
    from emoasr_amd.recurrence import lstm_layer_bwd, lstm_layer_fwd
    U, B, nin, H = 4, 3, 16, 32
    g = torch.Generator().manual_seed(21)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    x, w_ih, w_hh, bias, dh = rn(U, B, nin), rn(4 * H, nin, sc=0.3), rn(4 * H, H, sc=H ** -0.5), rn(4 * H, sc=0.3), rn(U, B, H, sc=0.5)
    h0, c0 = (rn(B, H, sc=0.5), rn(B, H, sc=0.5)) if with_state else (None, None)
    up = lambda t: None if t is None else t.to(dev)
    ops.split_products(split)
    try:
        hseq, cseq, gact = lstm_layer_fwd(up(x), up(w_ih), up(w_hh), up(bias), up(h0), up(c0))
        grads = [torch.zeros(4 * H, nin, device=dev), torch.zeros(4 * H, H, device=dev), torch.zeros(4 * H, device=dev),
                 torch.zeros(4 * H, device=dev)]
        dx = lstm_layer_bwd(up(dh), up(x), hseq, cseq, gact, up(h0), up(c0), up(w_ih), up(w_hh), *grads)
        torch.cuda.synchronize()
    finally:
        ops.split_products(False)
    leaves = [t.double().requires_grad_(True) for t in (x, w_ih, w_hh, bias)]
    f = R.seq_fwd(leaves[0] @ leaves[1].t() + leaves[3], leaves[2], h0, c0)
    (f.h * dh.double()).sum().backward()
    want = {"hseq": f.h.detach(), "cseq": f.c.detach(), "dx": leaves[0].grad, "g_w_ih": leaves[1].grad, "g_w_hh": leaves[2].grad,
            "g_b_ih": leaves[3].grad, "g_b_hh": leaves[3].grad}
    got = {"hseq": hseq, "cseq": cseq, "dx": dx, "g_w_ih": grads[0], "g_w_hh": grads[1], "g_b_ih": grads[2], "g_b_hh": grads[3]}
    res = {k: float((got[k].cpu().double() - want[k]).abs().max()) / (1e-3 * float(want[k].abs().max())) for k in want}
    _report(f"layer {'f32x3' if split else 'f32'}", with_state, res)
