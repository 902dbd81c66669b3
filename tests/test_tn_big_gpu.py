"""The eight-wave 256x256 weight-gradient tile (csrc/gemm_big_tn.hip, option "tn_big") against the 128x128 kernel it replaces.

Reference for every case: a.double().t() @ b.double() of the same bf16 inputs plus the random initial contents of `out`, and
a.double().sum(0) for the bias gradient.  Yardstick: the old kernel on the same inputs (tn_big = 0).  error = max |got - ref| over
the reference's largest magnitude; the new kernel's error must be at most max(4 x the old kernel's, 2e-6), for products and bias
sums alike: both kernels form f32 sums of the same exact bf16 products in different chunkings and slice counts (emulated on the
CPU: errors 0 to 5.3e-7, ratio between two orders 0.7 to 2.3), while a wrong or missing term is 1e-3 and up; the floor is there
because the old kernel's error can be exactly 0 at small K.  Both errors are printed per case.

The Conv2d weight gradient (B rows gathered through the convolution's geometry) is held to the same bar against
ops.conv2_wgrad with tn_big = 0, through the segmented entry point with one and with five micro-batches."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LAYER = [(256, 1024, 1), (1024, 256, 1), (256, 256, 1), (512, 256, 1), (256, 256, 1), (256, 256, 0), (768, 256, 1), (256, 1024, 1),
         (1024, 256, 1)]   # (N1, N2, long reduction?) -- the products of test_gemm_tn_grouped_layer_shapes; entry 5 reduces over R rows


@pytest.fixture(autouse=True)
def _seed_and_options():
    from emoasr_amd import lib
    torch.manual_seed(4321)
    yield
    for name in ("tn_big", "tn_big_blocks"):   # (whatever a test left behind)
        lib.set_option(name, lib.option_default(name))


def _err(got, ref):
    assert torch.isfinite(got).all()
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def _make(dev, n1, n2, k, colsum, alpha, lda=None):
    """one problem: a [k, lda] with finite garbage in the columns n1..lda, b, random out (+ a guard row) and bias sums (+ guard)"""
    lda = lda or n1
    a_full = torch.randn(k, lda, device=dev).to(torch.bfloat16)
    if lda > n1:
        a_full[:, n1:] = 1e4
    a = a_full[:, :n1]
    b = (torch.randn(k, n2, device=dev) * k ** -0.5).to(torch.bfloat16)
    out0 = torch.randn(n1 + 1, n2, device=dev)
    cs0 = torch.randn(n1 + 8, device=dev) if colsum else None
    ref = out0[:n1].double() + alpha * (a.double().t() @ b.double())
    ref_cs = cs0[:n1].double() + alpha * a.double().sum(0) if colsum else None
    return dict(a=a, b=b, out0=out0, cs0=cs0, alpha=alpha, ref=ref, ref_cs=ref_cs, n1=n1)


def _run(problems, big, blocks=0, call="grouped"):
    from emoasr_amd import lib, ops
    outs, css, args = [], [], []
    for p in problems:
        out = p["out0"].clone()
        cs = None if p["cs0"] is None else p["cs0"].clone()
        outs.append(out)
        css.append(cs)
        args.append((p["a"], p["b"], out[:p["n1"]], p["alpha"], None if cs is None else cs[:p["n1"]], p["alpha"]))
    with lib.options(tn_big=big, tn_big_blocks=blocks):
        if call == "grouped":
            ops.gemm_tn_grouped(args)
        else:
            for a, b, out, alpha, cs, s in args:
                ops.gemm_tn(a, b, out=out, alpha=alpha, accumulate=True, colsum=cs, colsum_scale=s)
        torch.cuda.synchronize()
    return outs, css


def _check(problems, what, blocks=0, call="grouped"):
    old_o, old_c = _run(problems, 0, call=call)
    new_o, new_c = _run(problems, 1, blocks, call=call)
    for i, p in enumerate(problems):
        n1 = p["n1"]
        e_old, e_new = _err(old_o[i][:n1], p["ref"]), _err(new_o[i][:n1], p["ref"])
        print(f"{what} product {i} ({n1} x {p['b'].shape[1]}, K {p['a'].shape[0]}): old {e_old:.3e} new {e_new:.3e}")
        assert e_new <= max(4 * e_old, 2e-6), (what, i, e_old, e_new)
        assert torch.equal(new_o[i][n1], p["out0"][n1]), f"{what} product {i}: guard row written"
        if p["cs0"] is not None:
            c_old, c_new = _err(old_c[i][:n1], p["ref_cs"]), _err(new_c[i][:n1], p["ref_cs"])
            print(f"{what} bias sum {i}: old {c_old:.3e} new {c_new:.3e}")
            assert c_new <= max(4 * c_old, 2e-6), (what, i, c_old, c_new)
            assert torch.equal(new_c[i][n1:], p["cs0"][n1:]), f"{what} bias sum {i}: guard written"


def _layer(dev, k, r, colsum, alpha):
    return [_make(dev, n1, n2, k if long_k else r, colsum and long_k, alpha) for n1, n2, long_k in LAYER]


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("colsum", [1, 0], ids=["colsum", "nocolsum"])
def test_layer_shapes(dev, colsum, alpha):
    _check(_layer(dev, 3001, 411, colsum, alpha), "layer K=3001")


def test_layer_shapes_long(dev):
    _check(_layer(dev, 35145, 411, 1, 0.5), "layer K=35145")


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("colsum", [1, 0], ids=["colsum", "nocolsum"])
@pytest.mark.parametrize("k", [35145, 777])
def test_head(dev, k, colsum, alpha):
    """the vocabulary head: ragged N1 under a padded lda; the columns N1..lda of A hold 1e4, the edge tile must mask them"""
    _check([_make(dev, 10000, 256, k, colsum, alpha, lda=10048)], f"head K={k}")


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("colsum", [1, 0], ids=["colsum", "nocolsum"])
def test_mixed_group(dev, colsum, alpha):
    """one 64-wide product among 256-multiples: two launches in one call"""
    shapes = [(256, 256), (512, 64), (1024, 256), (256, 1024)]
    _check([_make(dev, n1, n2, 3001, colsum, alpha) for n1, n2 in shapes], "mixed group")


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("colsum", [1, 0], ids=["colsum", "nocolsum"])
@pytest.mark.parametrize("k", [40, 1])
def test_short_reductions(dev, k, colsum, alpha):
    _check([_make(dev, n1, n2, k, colsum, alpha) for n1, n2 in [(256, 256), (1024, 256), (256, 1024)]], f"K={k}")


@pytest.mark.parametrize("blocks", [64, 128, 192, 256, 320, 512, 1024])
def test_block_budgets(dev, blocks):
    """option tn_big_blocks takes 64 .. 1024: both ends, the tuning candidates and two in between"""
    _check(_layer(dev, 3001, 411, 1, 1.0), f"layer, {blocks} blocks", blocks=blocks)


@pytest.mark.parametrize("colsum", [1, 0], ids=["colsum", "nocolsum"])
def test_plain_entry(dev, colsum):
    """emoasr_gemm_tn dispatches by the same rule: the front-end Linear's 256 x 4864 gradient, and the head"""
    _check([_make(dev, 256, 4864, 3001, colsum, 1.0), _make(dev, 10000, 256, 777, colsum, 0.5, lda=10048)], "plain", call="plain")



# ---- Conv2d(C -> C, k3, s2) weight gradient ---------------------------------------------------------------------------------------
def _conv_case(dev, B, T1, F1, C):
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    y1 = torch.randn(B, T1, F1, C, device=dev).to(torch.bfloat16)
    dy2 = (torch.randn(B, T2, F2, C, device=dev) * (B * T2 * F2) ** -0.5).to(torch.bfloat16)
    ref = torch.zeros(C, 9, C, device=dev, dtype=torch.float64)
    d2 = dy2.double().reshape(-1, C)
    for kh in range(3):
        for kw in range(3):
            patch = y1.double()[:, kh:kh + 2 * T2 - 1:2, kw:kw + 2 * F2 - 1:2, :].reshape(-1, C)
            ref[:, kh * 3 + kw] = d2.t() @ patch
    return dy2, y1, ref.reshape(C, 9 * C), d2.sum(0)


def _conv_check(dev, segs, what, run_old, run_new):
    """segs: _conv_case tuples accumulated into one dw / dbias (random initial contents, guards behind both)"""
    from emoasr_amd import lib
    C = segs[0][1].shape[-1]
    dw0, db0 = torch.randn(C + 1, 9 * C, device=dev), torch.randn(C + 8, device=dev)
    ref_w = dw0[:C].double() + sum(s[2] for s in segs)
    ref_b = db0[:C].double() + sum(s[3] for s in segs)
    res = {}
    for name, big, fn in (("old", 0, run_old), ("new", 1, run_new)):
        dw, db = dw0.clone(), db0.clone()
        with lib.options(tn_big=big):
            fn([(s[0], s[1]) for s in segs], dw[:C], db[:C])
            torch.cuda.synchronize()
        res[name] = (_err(dw[:C], ref_w), _err(db[:C], ref_b))
        assert torch.equal(dw[C], dw0[C]) and torch.equal(db[C:], db0[C:]), f"{what} {name}: guard written"
    print(f"{what}: dw old {res['old'][0]:.3e} new {res['new'][0]:.3e}   dbias old {res['old'][1]:.3e} new {res['new'][1]:.3e}")
    assert res["new"][0] <= max(4 * res["old"][0], 2e-6), (what, res)
    assert res["new"][1] <= max(4 * res["old"][1], 2e-6), (what, res)


def _plain_calls(segs, dw, db):
    from emoasr_amd import ops
    for dy2, y1 in segs:
        ops.conv2_wgrad(dy2, y1, dw, dbias=db, accumulate=True)


def _seg_call(segs, dw, db):
    from emoasr_amd import ops
    ops.conv2_wgrad_seg(segs, dw, dbias=db)


@pytest.mark.parametrize("shape", [(3, 41, 39, 256), (5, 97, 39, 256), (1, 7, 7, 256), (2, 30, 11, 512)], ids=str)
def test_conv2_wgrad(dev, shape):
    """(the 256 tile serves the segmented entry point only: one segment of it against the plain call on the old kernel)"""
    _conv_check(dev, [_conv_case(dev, *shape)], f"conv2 wgrad {shape}", _plain_calls, _seg_call)


def test_conv2_wgrad_five_segments(dev):
    """five micro-batches of different B and T1 in one launch against five launches of the old kernel into one buffer"""
    segs = [_conv_case(dev, B, T1, 39, 256) for B, T1 in [(3, 41), (5, 97), (1, 7), (2, 30), (4, 63)]]
    _conv_check(dev, segs, "conv2 wgrad, 5 segments", _plain_calls, _seg_call)

