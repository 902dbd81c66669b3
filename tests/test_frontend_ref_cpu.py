"""tests/frontend_ref.py pinned on the CPU: the float64 restatement against torch.nn.functional.conv2d + autograd, the
preconditions of every integer case (equality on the GPU is only meaningful where every summation order is exact), each mutant of
the float32 model leaving its bound or breaking equality on a named case (fold_no_round excepted: the issue's own bound admits
it, see test_rounding_of_dy1_in_the_fold), and the constants tests/test_frontend_kernels_gpu.py
quotes."""
import pytest
import torch
import torch.nn.functional as Fn

from tests import frontend_ref as R

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


def _nchw_w1(w1):
    return w1.reshape(-1, 1, 3, 3)


def _nchw_w2(w):
    N, C = w.shape[0], w.shape[1] // 9
    return w.reshape(N, 3, 3, C).permute(0, 3, 1, 2)


# (B, T, F, C): T1 / F1 = 3 (the smallest), even T1 and F1 (a last row / column of dy1 without a tap), even T and F, C = 8
PIN_SHAPES = [(1, 7, 7, 8), (2, 9, 10, 8), (2, 10, 9, 16), (3, 12, 11, 8), (2, 14, 13, 8), (1, 13, 20, 24)]


@pytest.mark.parametrize("B,T,F,C", PIN_SHAPES)
def test_reference_against_autograd(B, T, F, C):
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + F)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x, w1, b1, w2, b2 = rn(B, T, F), rn(C, 9).requires_grad_(), rn(C).requires_grad_(), rn(C, 9 * C).requires_grad_(), rn(C).requires_grad_()
    z1 = Fn.conv2d(x[:, None], _nchw_w1(w1), b1, stride=2)
    a1 = torch.relu(z1).detach().requires_grad_()
    z2 = Fn.conv2d(a1, _nchw_w2(w2), b2, stride=2)
    T1, F1, T2, F2 = R.out_len(T), R.out_len(F), R.out_len(R.out_len(T)), R.out_len(R.out_len(F))
    assert z1.shape == (B, C, T1, F1) and z2.shape == (B, C, T2, F2)
    dy2 = rn(B, T2, F2, C)
    torch.relu(z2).backward((dy2 * (z2.permute(0, 2, 3, 1) > 0)).permute(0, 3, 1, 2))      # dy2: the gradient w.r.t. the pre-ReLU z2
    dy2m = (dy2 * (z2.permute(0, 2, 3, 1) > 0)).reshape(-1, C).detach()
    dy1_auto = (a1.grad * (a1 > 0)).permute(0, 2, 3, 1)
    z1.backward(dy1_auto.permute(0, 3, 1, 2))
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)

    y1, _ = R.conv1_fwd(x, w1.detach(), b1.detach())
    close(y1, a1.detach().permute(0, 2, 3, 1))
    y2, _ = R.conv2_fwd(y1, w2.detach(), b2.detach())
    close(y2, torch.relu(z2).detach().permute(0, 2, 3, 1).reshape(-1, C))
    y2n, _ = R.conv2_fwd(y1, w2.detach(), None, act=R.ACT_NONE, alpha=0.5)
    close(y2n, 0.5 * (z2.detach() - b2.detach()[None, :, None, None]).permute(0, 2, 3, 1).reshape(-1, C))
    dy1, _ = R.conv2_dgrad(dy2m, w2.detach(), y1)
    close(dy1, dy1_auto)
    close(R.conv2_dgrad(dy2m, R.wt_of(w2.detach()), y1, layout="wt")[0], dy1_auto)
    close(R.col2im(dy2m @ w2.detach(), y1)[0], dy1_auto)
    dw, db, _, _ = R.conv2_wgrad([(dy2m, y1)])
    close(dw, w2.grad)
    close(db, b2.grad)
    if B > 1:      # two segments are one sum
        M1 = T2 * F2
        dws, dbs, _, _ = R.conv2_wgrad([(dy2m[:M1], y1[:1]), (dy2m[M1:], y1[1:])])
        close(dws, w2.grad)
        close(dbs, b2.grad)
    dw1, db1, _, _ = R.conv1_wgrad(x, dy1_auto)
    close(dw1, w1.grad)
    close(db1, b1.grad)
    # the fold: conv1_wgrad of the ROUNDED data gradient
    f = R.conv2_dgrad_w1(dy2m, R.wt_of(w2.detach()), y1, x)
    want = R.conv1_wgrad(x, dy1_auto.to(BF).double())
    close(f[0], want[0])
    close(f[1], want[1])
    assert not torch.equal(f[0], dw1)


def test_an_even_last_row_has_no_tap():
    """T1 = F1 = 6: the last row and column of dy1 are written zeros of the reference, whatever dy2 holds"""
    inp = R.conv2_inputs(("c2d", "int", 2, 6, 6, 256), "bf16")
    dy1 = R.ev(inp, "c2d", F64)[0]
    assert bool((dy1[:, 5] == 0).all()) and bool((dy1[:, :, 5] == 0).all()) and bool((dy1[:, :5, :5] != 0).any())


INT_TABLES = (("c1f", R.C1F_INT, R.conv1_inputs, ({},)),
              ("c1w", R.C1W_INT, R.conv1_inputs, ({},)),
              ("c2f", R.C2F_INT, R.conv2_inputs, ({}, {"bias": False}, {"act": R.ACT_NONE}, {"alpha": 0.5})),
              ("c2d", R.C2D_INT, R.conv2_inputs, ({}, {"layout": "wt"})),
              ("col2im", R.C2D_INT, R.conv2_inputs, ({},)),
              ("c2w", R.C2W_INT + R.C2W_SEG_INT, R.wgrad_inputs, ({},)),
              ("w1", R.W1_INT + list(R.W1_TILES.values()), R.fold_inputs, ({},)))


@pytest.mark.parametrize("op,table,make,variants", INT_TABLES, ids=[t[0] for t in INT_TABLES])
def test_integer_preconditions_over_the_whole_table(op, table, make, variants):
    """stored values bf16-exact integers (<= 256), every sum |term| below 2^24: any float32 order is exact"""
    for case in table:
        for dname in (("bf16",) if op == "w1" else ("bf16", "f32")):
            inp = make(case, dname)
            for kw in variants:
                R.assert_exact(inp, op, **kw)
            for t in (v for v in inp.__dict__.values() if torch.is_tensor(v)):
                assert bool((t.to(BF).float() == t).all())


def test_sparse_weight_meets_every_tap_and_channel_once():
    for C in (32, 64, 256, 512):
        w = R.sparse_w2(C, torch.Generator().manual_seed(C)).reshape(C, 9, C)
        assert bool(((w != 0).sum(0) == 1).all()) and bool(((w != 0).sum(2) == 1).all()) and float(w.abs().max()) == 2
        assert torch.equal(R.wt_of(w.reshape(C, 9 * C)).reshape(C, 9, C), w.permute(2, 1, 0))


def _model_leaves(inp, op, mutant, k=0, **kw):
    """the float32 model inside its bound, the mutant outside (randn) -- or equal / unequal to the reference (int)"""
    good = R.ev(inp, op, F32, **kw)[k]
    bad = R.ev(inp, op, F32, tap=R.MUTANTS[mutant], **kw)[k]
    if inp.kind == "int":
        ref = R.ev(inp, op, F64, **kw)[k]
        assert torch.equal(good.double(), ref) and not torch.equal(bad.double(), ref), (inp.case, op, mutant)
    else:
        out = (lambda t: t.to(inp.dtype).float()) if op in ("c1f", "c2f", "c2d", "col2im") else (lambda t: t)
        assert R.check(inp, op, k, out(good), **kw) <= 1.0 < R.check(inp, op, k, out(bad), **kw), (inp.case, op, mutant)


MUTANT_CASES = [
    ("stride1", "c1f", R.conv1_inputs, ("c1f", "int", 3, 10, 83, 256), "f32", {}),
    ("stride1", "c2f", R.conv2_inputs, ("c2f", "randn", 2, 6, 5, 64), "bf16", {}),
    ("stride1", "c2w", R.wgrad_inputs, ("c2w", "int", ((2, 9),), 7, 128), "bf16", {}),
    ("tap_order", "c1f", R.conv1_inputs, ("c1f", "randn", 1, 7, 131, 8), "bf16", {}),
    ("tap_order", "c1w", R.conv1_inputs, ("c1w", "int", 3, 19, 20, 8), "bf16", {}),
    ("tap_order", "c2f", R.conv2_inputs, ("c2f", "int", 2, 5, 6, 64), "bf16", {}),
    ("tap_order", "c2d", R.conv2_inputs, ("c2d", "randn", 2, 5, 6, 64), "bf16", {}),
    ("tap_order", "col2im", R.conv2_inputs, ("c2d", "int", 2, 5, 6, 64), "f32", {}),
    ("no_parity", "c2d", R.conv2_inputs, ("c2d", "int", 2, 6, 5, 256), "bf16", {}),
    ("no_parity", "c2d", R.conv2_inputs, ("c2d", "randn", 2, 5, 6, 64), "f32", {"layout": "wt"}),
    ("no_parity", "col2im", R.conv2_inputs, ("c2d", "int", 2, 6, 5, 256), "bf16", {}),
    ("last_row", "c1f", R.conv1_inputs, ("c1f", "int", 3, 10, 83, 256), "bf16", {}),
    ("last_row", "c1w", R.conv1_inputs, ("c1w", "int", 3, 20, 19, 8), "f32", {}),
    ("last_row", "c2f", R.conv2_inputs, ("c2f", "int", 2, 6, 5, 256), "bf16", {}),
    ("wt_as_w", "c2d", R.conv2_inputs, ("c2d", "int", 2, 5, 6, 64), "bf16", {"layout": "wt"}),
    ("wt_as_w", "c2d", R.conv2_inputs, ("c2d", "randn", 2, 5, 6, 64), "bf16", {"layout": "wt"}),
    ("wt_as_w", "w1", R.fold_inputs, ("w1", "int", 2, 9, 12, 512), "bf16", {}),
    ("fold_slice", "w1", R.fold_inputs, ("w1", "int", 2, 11, 12, 256), "bf16", {}),
]


@pytest.mark.parametrize("mutant,op,make,case,dname,kw", MUTANT_CASES, ids=[f"{m[0]}-{m[1]}-{R.case_id(m[3])}" for m in MUTANT_CASES])
def test_each_mutant_is_seen(mutant, op, make, case, dname, kw):
    _model_leaves(make(case, dname), op, mutant, **kw)


def test_last_row_mutant_needs_an_even_length():
    """at odd T the windows anchored at the end are the windows: the mutant is the model (the case tables hold both parities)"""
    inp = R.conv1_inputs(("c1f", "int", 3, 11, 83, 256), "bf16")
    assert torch.equal(R.ev(inp, "c1f", F32, tap=R.MUTANTS["last_row"])[0], R.ev(inp, "c1f", F32)[0])


def test_rounding_of_dy1_in_the_fold():
    """a fold on the UNROUNDED dy1 is not the operation: on the randn case it differs from the model that rounds, while on every
    integer case dy1 is bf16-exact and the two are equal -- there the comparison does not depend on where, or whether, the kernel
    rounds.  The f64 bound of the randn cases admits either by its 2^-8 sum |dy1 x| term.  So NOTHING in the suite pins the place
    of the rounding on the device: the fold_no_round mutant neither leaves a bound nor breaks an equality the GPU module asserts;
    what is shown here is only that the model rounds and that the 2^-8 term is needed, not slack."""
    inp = R.fold_inputs(R.W1_RANDN[0])
    good, bad = R.ev(inp, "w1", F32), R.ev(inp, "w1", F32, tap=R.MUTANTS["fold_no_round"])
    assert not torch.equal(good[0], bad[0]) and not torch.equal(good[1], bad[1])
    for k in (0, 1):
        assert R.check(inp, "w1", k, good[k]) <= 1.0
    # without the 2^-8 term the unrounded fold is outside the rest of the bound: the term is needed, not slack
    ref = R.ev(inp, "w1", F64)
    assert float((bad[0].double() - ref[0]).abs().max()) > 16 * float((good[0].double() - ref[0]).abs().max())
    inp = R.fold_inputs(("w1", "int", 2, 13, 14, 256))
    assert torch.equal(R.ev(inp, "w1", F32)[0], R.ev(inp, "w1", F32, tap=R.MUTANTS["fold_no_round"])[0])


def test_f32x3_constant():
    """F32X3_C: |a b - (ah bh + ah bl + al bh)| <= c 2^-16 |a b| with c = 3.03, on random operands (and not by a wide margin: the
    three dropped terms are 2^-16 each at worst, 1.8 is met)"""
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(1 << 18, generator=g), torch.randn(1 << 18, generator=g)
    sp = lambda v: (v.to(BF).float(), (v - v.to(BF).float()).to(BF).float())
    (ah, al), (bh, bl) = sp(a), sp(b)
    kept = ah.double() * bh.double() + ah.double() * bl.double() + al.double() * bh.double()
    worst = float(((a.double() * b.double() - kept).abs() / (a.double() * b.double()).abs()).max()) / 2.0 ** -16
    assert 1.0 < worst <= R.F32X3_C, worst
    assert (2.0 ** -16 * 3) * (1 + 2.0 ** -7) <= R.F32X3_C * 2.0 ** -16


def test_constants_the_gpu_module_quotes():
    assert [c[2] * R.out_len(c[3]) * R.out_len(c[4]) for c in R.C2F_EDGE] == list(R.C2F_M)
    assert [R.class_rows(*c[2:5])[3][0] for c in R.C2D_ONE] == [127, 128, 129, 191, 192, 193, 255, 256, 257]
    assert [R.class_rows(*c[2:5])[0][0] for c in R.C2D_HEAVY] == [126, 128, 130, 190, 192, 194, 254, 256, 258, 129, 189, 195, 255, 258]
    assert [R.class_rows(2, 3, 3)[k][0] for k in range(4)] == [8, 4, 4, 2] and [t for _, t in R.class_rows(2, 3, 3)] == [4, 2, 2, 1]
    for tiles, case in R.W1_TILES.items():
        assert R.class_tiles(case[2], R.out_len(case[3]), R.out_len(case[4]), 128) == tiles
    # the 64-tile shape: the last rows of the last class (the 64th fold slice) hold non-zero dy1
    inp = R.fold_inputs(R.W1_TILES[64])
    assert inp.T1 % 2 == 1 and inp.F1 % 2 == 1 and bool((R.ev(inp, "w1", F64)[4][-1, inp.T1 - 2, 1::2] != 0).any())
    assert all(R.class_tiles(c[2], R.out_len(c[3]), R.out_len(c[4]), bm) == 4 for c in R.W1_INT[:64] for bm in (128, 192, 256))
    rows = lambda c: sum(B * R.out_len(T1) * R.out_len(c[3]) for B, T1 in c[2])
    assert [rows(c) for c in R.C2W_INT[:11]] == list(R.C2W_K) + [999]
    assert all((B * R.out_len(T1) * 3) % 32 for B, T1 in R.C2W_SEGS) and len(R.C2W_SEGS) == 8
    # a bf16 output of the sparse weight: 9 taps x 2 x 7 + a bias of 4 <= 256; a data gradient 4 x 2 x 7
    assert 9 * 2 * 7 + 4 <= 256 and 4 * 2 * 7 <= 256
