"""Per-kernel parity: every C-ABI entry point against a plain PyTorch fp32 expression of the
same op (tolerances: f32 mode tight; bf16 mode relative to bf16 rounding of the operands)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _tol(dtype, f32=2e-5, bf16=2e-2):
    return f32 if dtype == torch.float32 else bf16


def _close(got, ref, tol, what=""):
    got = got.float()
    ref = ref.float()
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def _rnd(dev, *shape, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).to(dtype)


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(1234)


@pytest.fixture(params=[1, 0], ids=["tr", "notr"])
def tr_mode(request):
    from emoasr_amd import lib
    with lib.options(tr_read=request.param):
        yield request.param


# ---------------------------------------------------------------- GEMM NT
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N,K", [(300, 256, 256), (1000, 1024, 256), (77, 1000, 256), (130, 256, 4864),
                                   (4100, 256, 1024), (64, 64, 32)])
def test_gemm_nt_plain(dev, dtype, M, N, K):
    from emoasr_amd import ops
    a, b = _rnd(dev, M, K, dtype=dtype), _rnd(dev, N, K, dtype=dtype, scale=K ** -0.5)
    out = ops.gemm_nt(a, b)
    _close(out, a.float() @ b.float().t(), _tol(dtype), f"gemm_nt {M}x{N}x{K}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_gemm_nt_epilogue(dev, dtype):
    from emoasr_amd import ops
    M, N, K = 333, 512, 256
    a, b = _rnd(dev, M, K, dtype=dtype), _rnd(dev, N, K, dtype=dtype, scale=K ** -0.5)
    bias = _rnd(dev, N)
    res = _rnd(dev, M, N, dtype=dtype)
    acc = a.float() @ b.float().t()
    # bias + swish + pre_out + residual
    pre = torch.empty(M, N, device=dev, dtype=dtype)
    out = ops.gemm_nt(a, b, bias=bias, act=ops.ACT_SWISH, pre_out=pre, residual=res, res_scale=0.5, alpha=2.0)
    pre_ref = 2.0 * acc + bias
    _close(pre, pre_ref, _tol(dtype), "pre_out")
    _close(out, res.float() + 0.5 * F.silu(pre_ref), _tol(dtype), "swish+res")
    # relu, f32 output
    out = ops.gemm_nt(a, b, bias=bias, act=ops.ACT_RELU, out_f32=True)
    assert out.dtype == torch.float32
    _close(out, F.relu(acc + bias), _tol(dtype), "relu f32out")
    # derivative epilogue: acc * swish'(u)
    u = _rnd(dev, M, N, dtype=dtype)
    out = ops.gemm_nt(a, b, dact_pre=u, dact=ops.ACT_SWISH)
    uf = u.float()
    s = torch.sigmoid(uf)
    _close(out, acc * (s * (1 + uf * (1 - s))), _tol(dtype), "dswish")
    out = ops.gemm_nt(a, b, dact_pre=u, dact=ops.ACT_RELU)
    _close(out, acc * (uf > 0).float(), _tol(dtype), "drelu")


def test_dropout_consistency(dev):
    """GEMM epilogue dropout == scale_dropout kernel mask (same seed, same linear index)."""
    from emoasr_amd import ops
    M, N, K, p = 200, 256, 64, 0.25
    a, b = _rnd(dev, M, K), _rnd(dev, N, K)
    plain = ops.gemm_nt(a, b)
    dropped = ops.gemm_nt(a, b, drop_p=p, seed=77)
    mask = ops.scale_dropout(torch.ones(M, N, device=dev), 1.0, p, 77)
    _close(dropped, plain * mask, 1e-6, "dropout mask")
    frac = (mask == 0).float().mean().item()
    assert abs(frac - p) < 0.02, f"drop fraction {frac}"
    kept = mask[mask != 0]
    assert torch.allclose(kept, torch.full_like(kept, 1 / (1 - p)))
    mask2 = ops.scale_dropout(torch.ones(M, N, device=dev), 1.0, p, 78)
    assert (mask2 != mask).any()


# ---------------------------------------------------------------- GEMM TN
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("K,N1,N2", [(1000, 256, 256), (3001, 1024, 256), (777, 1000, 256), (500, 256, 2304),
                                     (64, 64, 64)])
def test_gemm_tn(dev, dtype, tr_mode, K, N1, N2):
    from emoasr_amd import ops
    a, b = _rnd(dev, K, N1, dtype=dtype), _rnd(dev, K, N2, dtype=dtype, scale=K ** -0.5)
    ref = a.float().t() @ b.float()
    cs = torch.empty(N1, device=dev)
    out = ops.gemm_tn(a, b, alpha=0.5, colsum=cs, colsum_scale=2.0)
    _close(out, 0.5 * ref, _tol(dtype), f"gemm_tn {K}x{N1}x{N2}")
    _close(cs, 2.0 * a.float().sum(0), 1e-4, "fused colsum")
    ops.gemm_tn(a, b, out=out, alpha=1.0, accumulate=True, colsum=cs, colsum_scale=1.0)
    _close(out, 1.5 * ref, _tol(dtype), "gemm_tn accumulate")
    _close(cs, 3.0 * a.float().sum(0), 1e-4, "fused colsum accumulate")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_gemm_nn(dev, dtype, tr_mode):
    from emoasr_amd import ops
    for M, N, K in [(300, 256, 1024), (1000, 1024, 256), (77, 2304, 256), (130, 4864, 256), (64, 64, 32)]:
        a, b = _rnd(dev, M, K, dtype=dtype), _rnd(dev, K, N, dtype=dtype, scale=K ** -0.5)
        _close(ops.gemm_nn(a, b, alpha=0.5), 0.5 * (a.float() @ b.float()), _tol(dtype), f"gemm_nn {M}x{N}x{K}")
    # batched, ragged K with zero-padded rows (the attention-backward use)
    nb, nh, Mr, Kr, N = 2, 3, 45, 37, 64
    lda = 40
    a = torch.zeros(nb, nh, Mr, lda, device=dev, dtype=dtype)
    a[..., :Kr] = _rnd(dev, nb, nh, Mr, Kr, dtype=dtype)
    b = _rnd(dev, nb, Kr, nh * N, dtype=dtype)
    out = torch.zeros(nb, Mr, nh * N, device=dev, dtype=dtype)
    ops.gemm_nn_batched(a, b, out, Mr, N, Kr, lda, (nh * Mr * lda, Mr * lda), nh * N, (Kr * nh * N, N), nh * N,
                        (Mr * nh * N, N), nb, nh)
    ref = torch.einsum("bhmk,bkhn->bmhn", a[..., :Kr].float(), b.float().view(nb, Kr, nh, N)).reshape(nb, Mr, nh * N)
    _close(out, ref, _tol(dtype), "gemm_nn_batched")


def test_colsum(dev):
    from emoasr_amd import ops
    for dtype in DTYPES:
        x = _rnd(dev, 1001, 768, dtype=dtype)
        out = ops.colsum(x, scale=0.5)
        _close(out, 0.5 * x.float().sum(0), 1e-4, "colsum")
        ops.colsum(x, out=out, scale=1.0, accumulate=True)
        _close(out, 1.5 * x.float().sum(0), 1e-4, "colsum acc")


# ---------------------------------------------------------------- front-end convs
def _conv2_weight_repack(w):  # (C, C, 3, 3) -> (C, (kh,kw,c))
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def test_transpose_cast_batched(dev):
    """several f32 matrices -> their transposes in the compute dtype, one launch (the layer runtime's transposed weight copies);
    ragged shapes, a padded destination row stride"""
    from emoasr_amd import ops
    shapes = [(1024, 256), (768, 256), (33, 65), (1, 7), (512, 256)]
    for dt_ in (torch.bfloat16, torch.float32):
        srcs = [_rnd(dev, r, c) for r, c in shapes]
        dsts = [torch.full((c, r + (8 if i == 2 else 0)), float("nan"), device=dev, dtype=dt_)[:, :r] for i, (r, c) in enumerate(shapes)]
        ops.transpose_cast_batched(list(zip(srcs, dsts)))
        for s_, d_ in zip(srcs, dsts):
            assert torch.equal(d_, s_.t().to(dt_))


@pytest.mark.parametrize("B,T,Fd", [(3, 67, 80), (2, 70, 83), (1, 3, 3), (2, 1200, 80)])
def test_conv1_two_rows_per_block_equals_one_row_per_block(dev, B, T, Fd):
    """the training-shape conv1 kernel (bf16, C = 256: two output rows per block, two channels per thread) is bit-identical to the
    one-row kernel and matches torch's conv2d + ReLU; odd and even numbers of output rows, the smallest input"""
    from emoasr_amd import lib, ops
    C = 256
    x = _rnd(dev, B, T, Fd)
    w1, b1 = _rnd(dev, C, 1, 3, 3, scale=0.3), _rnd(dev, C, scale=0.1)
    ref = F.relu(F.conv2d(x.unsqueeze(1), w1, b1, stride=2)).permute(0, 2, 3, 1)
    outs = []
    for pair in (1, 0):
        with lib.options(conv1_pair=pair):
            outs.append(ops.conv1_fwd(x, w1.reshape(C, 9).contiguous(), b1, torch.bfloat16))
    assert torch.equal(outs[0], outs[1])
    _close(outs[0], ref, 1e-2, "conv1")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("T,Fd", [(67, 80), (70, 83), (9, 7)], ids=["odd-T1", "even-T1-F1", "tiny"])
def test_frontend(dev, dtype, tr_mode, T, Fd):
    from emoasr_amd import ops
    B, C = 3, 128
    x = _rnd(dev, B, T, Fd)
    w1, b1 = _rnd(dev, C, 1, 3, 3, scale=0.3), _rnd(dev, C, scale=0.1)
    w2, b2 = _rnd(dev, C, C, 3, 3, scale=(9 * C) ** -0.5), _rnd(dev, C, scale=0.1)
    xr = x.clone().requires_grad_(True)
    w1r, b1r, w2r, b2r = [t.clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
    y1_ref = F.relu(F.conv2d(xr.unsqueeze(1), w1r, b1r, stride=2))
    y1_ref.retain_grad()
    y2_ref = F.relu(F.conv2d(y1_ref, w2r, b2r, stride=2))
    g = torch.randn_like(y2_ref)
    y2_ref.backward(g)

    y1 = ops.conv1_fwd(x, w1.reshape(C, 9).contiguous(), b1, dtype)
    _close(y1, y1_ref.permute(0, 2, 3, 1), _tol(dtype, 1e-5, 1e-2), "conv1")
    w2p = _conv2_weight_repack(w2).to(dtype)
    y2 = ops.conv2_fwd(y1, w2p, bias=b2, act=ops.ACT_RELU)
    _close(y2, y2_ref.permute(0, 2, 3, 1), _tol(dtype), "conv2")
    # backward: dy2 (pre-relu grad), wgrad, dgrad via dcol + col2im, conv1 wgrad
    T2, F2 = y2.shape[1], y2.shape[2]
    dy2 = (g.permute(0, 2, 3, 1) * (y2_ref.permute(0, 2, 3, 1) > 0)).contiguous().to(dtype)
    dw2 = torch.empty(C, 9 * C, device=dev)
    db2 = torch.empty(C, device=dev)
    ops.conv2_wgrad(dy2, y1, dw2, dbias=db2)
    _close(dw2, _conv2_weight_repack(w2r.grad), _tol(dtype, 1e-4, 3e-2), "conv2 wgrad")
    _close(db2, b2r.grad, _tol(dtype, 1e-4, 3e-2), "conv2 bgrad")
    w2pt = w2p.t().contiguous()  # [(kh,kw,c), n]
    dcol = ops.gemm_nt(dy2.reshape(-1, C), w2pt)
    dy1 = ops.conv2_col2im(dcol, y1)
    # reference: grad wrt conv1 pre-relu output = y1_ref.grad * relu mask
    dy1_ref = (y1_ref.grad * (y1_ref > 0)).permute(0, 2, 3, 1)
    _close(dy1, dy1_ref, _tol(dtype, 1e-4, 3e-2), "col2im")
    # the same gradient as four parity-class implicit GEMMs (no im2col buffer)
    dy1_imp = ops.conv2_dgrad(dy2, w2p, y1)
    _close(dy1_imp, dy1_ref, _tol(dtype, 1e-4, 3e-2), "conv2 implicit dgrad")
    dw1 = torch.empty(C, 9, device=dev)
    db1 = torch.empty(C, device=dev)
    ops.conv1_wgrad(x, dy1, dw1, db1)
    _close(dw1, w1r.grad.reshape(C, 9), _tol(dtype, 1e-4, 3e-2), "conv1 wgrad")
    _close(db1, b1r.grad, _tol(dtype, 1e-4, 3e-2), "conv1 bgrad")


@pytest.mark.parametrize("bm", [0, 256, 192, 128])
@pytest.mark.parametrize("M,N,K", [(1000, 256, 128), (257, 512, 64), (5000, 256, 2304), (31, 256, 192), (3000, 1000, 512)])
def test_gemm_nt_big(dev, bm, M, N, K):
    """large-tile NT kernel (LDS-DMA staging, swizzled images, transposed accumulators) against f32 matmul of the same
    bf16 operands, every tile height, ragged last tiles"""
    from emoasr_amd import lib, ops
    a = _rnd(dev, M, K + 8, dtype=torch.bfloat16)[:, :K]  # lda != K
    b = _rnd(dev, N, K, dtype=torch.bfloat16, scale=K ** -0.5)
    bias = _rnd(dev, N, scale=0.5)
    with lib.options(big_bm=bm):
        for relu in (False, True):
            out = ops.gemm_nt_big(a, b, bias=bias, relu=relu)
            ref = a.float() @ b.float().t() + bias
            _close(out, F.relu(ref) if relu else ref, 1e-2, f"gemm_nt_big relu={relu}")
        out = ops.gemm_nt_big(a, b)
        _close(out, a.float() @ b.float().t(), 1e-2, "gemm_nt_big plain")


@pytest.mark.parametrize("M,N,K", [(700, 512, 256), (7029, 1024, 256), (333, 768, 128), (2000, 1000, 512)])
def test_gemm_nt_dispatch_to_large_tile_kernel(dev, M, N, K):
    """emoasr_gemm_nt hands wide bf16 products to the large-tile kernel; its epilogue (alpha, bias, saved pre-activation,
    Swish, dropout) must equal the 128x64 kernel's: identical dropout masks, values up to the accumulation order"""
    from emoasr_amd import lib, ops
    a = _rnd(dev, M, K, dtype=torch.bfloat16)
    b = _rnd(dev, N, K, dtype=torch.bfloat16, scale=K ** -0.5)
    bias = _rnd(dev, N, scale=0.5)
    outs = []
    for big in (1, 0):
        with lib.options(conv_big=big, big_min_tiles=1):
            pre = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            y = ops.gemm_nt(a, b, bias=bias, alpha=0.5, act=ops.ACT_SWISH, pre_out=pre, drop_p=0.1, seed=77)
            outs.append((y, pre, ops.gemm_nt(a, b)))
    (y1, p1, r1), (y0, p0, r0) = outs
    assert torch.equal(y1 == 0, y0 == 0), "dropout masks differ"
    _close(p1, 0.5 * (a.float() @ b.float().t()) + bias, 1e-2, "pre-activation")
    _close(p1, p0, 1e-2, "pre-activation vs 128x64")
    _close(y1, y0, 1e-2, "swish + dropout vs 128x64")
    _close(r1, r0, 1e-2, "plain")


@pytest.mark.parametrize("M,N,K", [(8200, 256, 1024), (9001, 256, 768), (8192, 256, 4864)])
def test_gemm_nt_long_reductions_on_one_column_tile(dev, M, N, K):
    """N = 256, K >= 512, many rows (the second feed-forward product, the front-end Linear of the stacked step): emoasr_gemm_nt
    takes the large-tile kernel, whose residual epilogue (x + res_scale * dropout(alpha * acc + bias), in place) must equal the
    64 x 64 kernel's -- same dropout mask, same values -- and the f32 product of the same operands"""
    from emoasr_amd import lib, ops
    a = _rnd(dev, M, K, dtype=torch.bfloat16)
    b = _rnd(dev, N, K, dtype=torch.bfloat16, scale=K ** -0.5)
    bias = _rnd(dev, N, scale=0.5)
    x0 = _rnd(dev, M, N, dtype=torch.bfloat16)
    outs = []
    for big in (2, 0):   # (2: N = 256 from K = 512 on; 1 takes K >= 2048 only)
        with lib.options(big_n256=big):
            x = x0.clone()
            ops.gemm_nt(a, b, out=x, bias=bias, residual=x, res_scale=0.5, drop_p=0.1, seed=91)   # in place
            outs.append((x, ops.gemm_nt(a, b, bias=bias, residual=x0, res_scale=0.5), ops.gemm_nt(a, b, bias=bias)))
    (x1, r1, p1), (x0_, r0, p0) = outs
    assert torch.equal(x1 == x0, x0_ == x0), "dropout masks differ"
    ref = a.float() @ b.float().t() + bias
    _close(p1, ref, 1e-2, "plain")
    _close(r1, x0.float() + 0.5 * ref, 1e-2, "residual")
    _close(x1, x0_, 1e-2, "residual + dropout vs 64x64")
    _close(r1, r0, 1e-2, "residual vs 64x64")
    kept = x1 != x0
    _close(x1[kept], (x0.float() + 0.5 * ref / 0.9)[kept], 2e-2, "kept elements")


@pytest.mark.parametrize("bm", [0, 256, 192, 128])
@pytest.mark.parametrize("B,T,Fd", [(3, 67, 80), (2, 70, 83), (5, 9, 7), (2, 300, 80)], ids=["odd", "even", "tiny", "long"])
def test_conv2_large_tile_kernels(dev, bm, B, T, Fd):
    """Conv2d(256 -> 256, k3, s2) forward and data gradient on the large-tile kernel == torch conv2d autograd, and the
    forward == the 128x64-tile implicit GEMM it replaces up to bf16 output rounding"""
    from emoasr_amd import lib, ops
    C = 256
    dtype = torch.bfloat16
    x = _rnd(dev, B, T, Fd)
    w1, b1 = _rnd(dev, C, 1, 3, 3, scale=0.3), _rnd(dev, C, scale=0.1)
    w2, b2 = _rnd(dev, C, C, 3, 3, scale=(9 * C) ** -0.5), _rnd(dev, C, scale=0.1)
    y1 = ops.conv1_fwd(x, w1.reshape(C, 9).contiguous(), b1, dtype)
    y1r = y1.float().permute(0, 3, 1, 2).clone().requires_grad_(True)   # the SAME bf16 input for the reference
    w2b = w2.to(dtype)
    y2_ref = F.relu(F.conv2d(y1r, w2b.float(), b2, stride=2))
    g = torch.randn_like(y2_ref)
    y2_ref.backward(g)
    w2p = _conv2_weight_repack(w2b)
    with lib.options(big_bm=bm):
        y2 = ops.conv2_fwd(y1, w2p, bias=b2, act=ops.ACT_RELU)
        with lib.options(conv_big=0):
            y2_old = ops.conv2_fwd(y1, w2p, bias=b2, act=ops.ACT_RELU)
        _close(y2, y2_ref.permute(0, 2, 3, 1), 1e-2, "conv2 big")
        _close(y2, y2_old, 1e-2, "conv2 big vs 128x64")
        dy2 = (g.permute(0, 2, 3, 1) * (y2_ref.permute(0, 2, 3, 1) > 0)).contiguous().to(dtype)
        wt = w2b.permute(1, 2, 3, 0).reshape(C, 9 * C).contiguous()
        dy1 = ops.conv2_dgrad_kc(dy2, wt, y1)
        # the reference consumes the same bf16 dy2
        y1r.grad = None
        y2_ref2 = F.conv2d(y1r, w2b.float(), b2, stride=2)
        y2_ref2.backward(dy2.float().permute(0, 3, 1, 2))
        dy1_ref = (y1r.grad * (y1r > 0)).permute(0, 2, 3, 1)
        _close(dy1, dy1_ref, 1.5e-2, "conv2 big dgrad")
        _close(dy1, ops.conv2_dgrad(dy2, w2p, y1), 1.5e-2, "conv2 big dgrad vs parity-class launches")


@pytest.mark.parametrize("B,T,C,K", [(3, 70, 256, 31), (2, 33, 256, 15), (2, 20, 144, 31), (1, 100, 512, 7), (4, 320, 256, 31)])
def test_fused_conv_module_kernels_are_bit_identical(dev, B, T, C, K):
    """csrc/convfused.hip against the separate launches it replaces (bf16): the LDS-staged depthwise convolution, GLU fused
    into it, and BatchNorm/Swish apply -> depthwise data gradient -> GLU backward + weight-gradient partials in one launch.
    Every intermediate is rounded at the same point, so all outputs must be EQUAL, not close."""
    from emoasr_amd import lib, ops
    dt_ = torch.bfloat16
    g = _rnd(dev, B * T, 2 * C, dtype=dt_)
    w, bias = _rnd(dev, C, K, scale=K ** -0.5), _rnd(dev, C, scale=0.1)
    gamma, beta = 1 + 0.1 * _rnd(dev, C), 0.1 * _rnd(dev, C)
    ds = _rnd(dev, B * T, C, dtype=dt_)
    nbt = torch.zeros((), device=dev, dtype=torch.int64)

    def unfused():
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        gl = ops.glu_fwd(g)
        c, mean, var = ops.dwconv_bn_stats_fwd(gl.view(B, T, C), w, bias, rm, rv, 0.1, nbt.clone())
        c_eval = ops.dwconv_fwd(gl.view(B, T, C), w, bias)
        dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        dc = ops.bn_swish_bwd(ds, c.view(B * T, C), mean, var, gamma, beta, 1e-5, dgam, dbet)
        dgl = ops.dwconv_bwd_x(dc.view(B, T, C), w)
        dw, db = torch.zeros(C, K, device=dev), torch.zeros(C, device=dev)
        ops.dwconv_bwd_w(dc.view(B, T, C), gl.view(B, T, C), dw, db, accumulate=True)
        dg = ops.glu_bwd(g, dgl.view(B * T, C))
        return dict(c=c, mean=mean, var=var, rm=rm, rv=rv, c_eval=c_eval, dgam=dgam, dbet=dbet, dw=dw, db=db, dg=dg, dgl=dgl)

    def fused():
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        c, mean, var = ops.glu_dwconv_fwd(g, B, T, w, bias, rm, rv, 0.1, nbt.clone(), True)
        c_eval = ops.glu_dwconv_fwd(g, B, T, w, bias, rm, rv, training=False)[0]
        dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        dw, db = torch.zeros(C, K, device=dev), torch.zeros(C, device=dev)
        dg = ops.conv_bwd_fused(ds, c.view(B * T, C), mean, var, gamma, beta, 1e-5, dgam, dbet, g, w, dw, db, B, T)
        return dict(c=c, mean=mean, var=var, rm=rm, rv=rv, c_eval=c_eval, dgam=dgam, dbet=dbet, dw=dw, db=db, dg=dg)

    with lib.options(dwconv_lds=0):
        ref = unfused()          # the round-1 kernels
    with lib.options(dwconv_lds=1):
        lds = unfused()          # same sequence, LDS-staged stencils
        got = fused()
    for k, v in ref.items():
        assert torch.equal(lds[k], v), f"LDS-staged dwconv: {k} differs"
        if k in got:
            assert torch.equal(got[k], v), f"fused: {k} differs (max {(got[k].float() - v.float()).abs().max().item():.3e})"


# ---------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("N,eps", [(256, 1e-5), (256, 1e-12), (64, 1e-5), (1024, 1e-5)])
def test_layernorm(dev, dtype, N, eps):
    from emoasr_amd import ops
    M = 517
    x = _rnd(dev, M, N, dtype=dtype) * 2 + 0.5
    g, b = _rnd(dev, N) + 1, _rnd(dev, N)
    xr, gr, br = x.float().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.layer_norm(xr, (N,), gr, br, eps)
    dy = _rnd(dev, M, N, dtype=dtype)
    dres = _rnd(dev, M, N, dtype=dtype)
    yr.backward(dy.float())
    y, mean, rstd = ops.layernorm_fwd(x, g, b, eps)
    _close(y, yr, _tol(dtype, 1e-5, 1e-2), "ln fwd")
    dg, db = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    dx = ops.layernorm_bwd(dy, x, g, mean, rstd, dres, dg, db)
    _close(dx, xr.grad + dres.float(), _tol(dtype, 1e-5, 1e-2), "ln dx")
    _close(dg, gr.grad, 1e-4, "ln dgamma")
    _close(db, br.grad, 1e-4, "ln dbeta")


# ---------------------------------------------------------------- attention
def _attn_ref(q, k, v, H, scale, pos, bu, bv, klens, causal):
    B, Tq, D = q.shape
    Tk = k.shape[1]
    dk = D // H
    qh = q.view(B, Tq, H, dk).transpose(1, 2)
    kh = k.view(B, Tk, H, dk).transpose(1, 2)
    vh = v.view(B, Tk, H, dk).transpose(1, 2)
    if bu is not None:
        qu = qh + bu.view(1, H, 1, dk)
    else:
        qu = qh
    scores = qu @ kh.transpose(-1, -2)
    if pos is not None:
        qv = qh + bv.view(1, H, 1, dk)
        ph = pos.view(-1, H, dk).transpose(0, 1)  # (H, 2T-1, dk)
        bd_full = qv @ ph.transpose(-1, -2).unsqueeze(0)  # (B,H,Tq,2T-1)
        i = torch.arange(Tq, device=q.device).view(-1, 1)
        j = torch.arange(Tk, device=q.device).view(1, -1)
        idx = (Tq - 1 - (i - j)).expand(B, H, Tq, Tk)
        scores = scores + torch.gather(bd_full, 3, idx)
    scores = scores * scale
    mask = torch.ones(B, 1, Tq, Tk, dtype=torch.bool, device=q.device)
    if klens is not None:
        mask = mask & (torch.arange(Tk, device=q.device).view(1, 1, 1, Tk) < klens.view(B, 1, 1, 1))
    if causal:
        mask = mask & torch.tril(torch.ones(Tq, Tk, dtype=torch.bool, device=q.device)).view(1, 1, Tq, Tk)
    scores = scores.masked_fill(~mask, torch.finfo(torch.float32).min)
    attn = torch.softmax(scores, -1).masked_fill(~mask, 0.0)
    return (attn @ vh).transpose(1, 2).reshape(B, Tq, D)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ["rel", "rel_long", "plain_mask", "causal", "cross"])
@pytest.mark.parametrize("mat", ["stored", True, False, "fused", "fused1"], ids=["stored", "gemmbwd", "recompute", "fused", "fused-single-pass"])
def test_attention(dev, dtype, tr_mode, case, mat):
    """"fused": the two-pass bf16 backward (attn_bwd_kv_kernel + attn_bwd_q_kernel, the default); "fused1": the single-pass kernel
    of rounds 2-3 (option attn_bwd_split = 0), kept as the A/B reference"""
    from emoasr_amd import lib, ops
    single = mat == "fused1"
    mat = "fused" if single else mat
    H, dk = 4, 64
    D = H * dk
    cfg = {"rel": (3, 75, 75, True, False, [75, 40, 9]), "rel_long": (2, 299, 299, True, False, [299, 170]),
           "plain_mask": (2, 50, 50, False, False, [50, 33]), "causal": (2, 41, 41, False, True, [41, 17]),
           "cross": (2, 21, 83, False, False, [83, 60])}[case]
    B, Tq, Tk, rel, causal, kl = cfg
    if mat == "fused" and (dtype != torch.bfloat16 or causal):
        pytest.skip("the single-pass backward is bf16 without causal mask; other cases run the paths above")
    klens = torch.tensor(kl, device=dev, dtype=torch.int32)
    qkv = _rnd(dev, B, Tq, 3 * D, dtype=dtype)
    if Tq == Tk:
        q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    else:
        q = _rnd(dev, B, Tq, D, dtype=dtype)
        kv = _rnd(dev, B, Tk, 2 * D, dtype=dtype)
        k, v = kv[..., :D], kv[..., D:]
    pos = _rnd(dev, 2 * Tq - 1, D, dtype=dtype) if rel else None
    bu = _rnd(dev, D, scale=0.5) if rel else None
    bv = _rnd(dev, D, scale=0.5) if rel else None
    scale = 1 / math.sqrt(dk)
    leaves = [t.float().clone().requires_grad_(True) if t is not None else None for t in (q, k, v, pos, bu, bv)]
    ref = _attn_ref(*leaves[:3], H, scale, leaves[3], leaves[4], leaves[5], klens, causal)
    dout = _rnd(dev, B, Tq, D, dtype=dtype)
    ref.backward(dout.float())
    st = None
    if mat == "stored":
        out, lse, st = ops.attn_fwd(q, k, v, H, scale, pos=pos, bias_u=bu, bias_v=bv, klens=klens, causal=causal,
                                    store_scores=True)
    else:
        out, lse = ops.attn_fwd(q, k, v, H, scale, pos=pos, bias_u=bu, bias_v=bv, klens=klens, causal=causal)
    tol = _tol(dtype, 2e-5, 2e-2)
    _close(out, ref, tol, f"attn fwd {case}")
    if Tq == Tk:
        dqkv = torch.zeros_like(qkv)
        dq, dk_, dv = dqkv[..., :D], dqkv[..., D:2 * D], dqkv[..., 2 * D:]
    else:
        dq = torch.zeros_like(q)
        dkv = torch.zeros_like(kv)
        dk_, dv = dkv[..., :D], dkv[..., D:]
    dpos = torch.zeros(2 * Tq - 1, D, device=dev) if rel else None
    dbu = torch.zeros(D, device=dev) if rel else None
    dbv = torch.zeros(D, device=dev) if rel else None
    with lib.options(attn_bwd_split=0 if single else 1):
        ops.attn_bwd(dout, out, lse, q, k, v, H, scale, dq, dk_, dv, pos=pos, bias_u=bu, bias_v=bv, klens=klens,
                     causal=causal, dpos=dpos, dbias_u=dbu, dbias_v=dbv, materialise=mat if mat == "fused" else bool(mat), st=st)
    btol = _tol(dtype, 1e-4, 4e-2)
    _close(dq, leaves[0].grad, btol, f"attn dq {case}")
    _close(dk_, leaves[1].grad, btol, f"attn dk {case}")
    _close(dv, leaves[2].grad, btol, f"attn dv {case}")
    if rel:
        _close(dpos, leaves[3].grad, btol, f"attn dpos {case}")
        _close(dbu, leaves[4].grad, btol, f"attn dbias_u {case}")
        _close(dbv, leaves[5].grad, btol, f"attn dbias_v {case}")


def test_attention_dropout(dev):
    """Dropout inside the fused kernel: forward/backward consistent with each other (finite
    differences are impossible with a random mask, so check linearity in V and the drop rate)."""
    from emoasr_amd import ops
    B, T, H, D = 2, 64, 4, 256
    q, k = _rnd(dev, B, T, D), _rnd(dev, B, T, D)
    v = torch.ones(B, T, D, device=dev)
    out0, _ = ops.attn_fwd(q, k, v, H, 0.125)
    out1, _ = ops.attn_fwd(q, k, v, H, 0.125, drop_p=0.5, seed=5)
    _close(out0, torch.ones_like(out0), 1e-5, "rows sum to one")
    assert (out1 - 1).abs().mean() > 0.01 and abs(out1.mean().item() - 1) < 0.05
    out2, _ = ops.attn_fwd(q, k, v, H, 0.125, drop_p=0.5, seed=5)
    assert torch.equal(out1, out2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_attention_keep_mask_bits_equal_the_inline_hash(dev, dtype):
    """emoasr_attn_dropmask (round 6): the keep mask hashed ONCE as bits gives the forward -- and both passes of the fused backward --
    exactly what hashing the counter-based mask inline gives: same outputs, bit for bit; the bits' drop rate is p"""
    from emoasr_amd import ops
    B, T, H, D, p = 3, 150, 4, 256, 0.3
    torch.manual_seed(3)
    qkv = (torch.randn(B, T, 3 * D, device=dev) * 0.5).to(dtype)
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    pos = (torch.randn(2 * T - 1, D, device=dev) * 0.5).to(dtype)
    bu, bv = torch.randn(D, device=dev) * 0.1, torch.randn(D, device=dev) * 0.1
    klens = torch.tensor([150, 131, 97], device=dev, dtype=torch.int32)
    mask = ops.attn_dropmask(q, k, H, klens=klens, drop_p=p, seed=11)
    torch.cuda.synchronize()
    bits = 0
    for b in range(B):
        n = int(klens[b])
        w = mask.view(B, T, H, -1)[b].cpu().numpy().astype("uint32")
        import numpy as np
        un = np.unpackbits(w.view("uint8"), axis=-1, bitorder="little")[..., :n]
        bits += un.mean() / B
    assert abs(bits - (1 - p)) < 0.01, bits
    kw = dict(pos=pos, bias_u=bu, bias_v=bv, klens=klens, drop_p=p, seed=11)
    out0, lse0 = ops.attn_fwd(q, k, v, H, 0.125, **kw)
    out1, lse1 = ops.attn_fwd(q, k, v, H, 0.125, keep_mask=mask, **kw)
    assert torch.equal(out0, out1) and torch.equal(lse0, lse1)
    if dtype == torch.bfloat16:
        dout = torch.randn(B, T, D, device=dev).to(dtype)
        res = []
        for km in (None, mask):
            dqkv = torch.empty_like(qkv)
            dpos = torch.zeros(2 * T - 1, D, device=dev)
            dbu, dbv = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
            ops.attn_bwd(dout, out0, lse0, q, k, v, H, 0.125, dqkv[..., :D], dqkv[..., D:2 * D], dqkv[..., 2 * D:], dpos=dpos,
                         dbias_u=dbu, dbias_v=dbv, materialise="fused", keep_mask=km, **kw)
            torch.cuda.synchronize()
            res.append((dqkv, dpos))
        assert torch.equal(res[0][0], res[1][0])
        _close(res[1][1], res[0][1], 1e-3, "dpos with the forward's mask")   # (float atomics: order differs from run to run)


@pytest.mark.parametrize("shape", [(3, 150), (2, 33), (5, 257)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_attention_fwd_block_staged_equals_per_wave_kernel(dev, shape, p):
    """attn_fwd4_kernel (round 6: four query tiles per workgroup share LDS-staged K / V tiles and a ring of position-band blocks)
    against attn_fwd_kernel (every wave fetches its own fragments): the same MFMA order, soft-max and mask -> outputs and
    log-sum-exp bit for bit, ragged key lengths and keep-mask bits included"""
    from emoasr_amd import lib, ops
    B, T = shape
    H, D = 4, 256
    torch.manual_seed(9)
    qkv = (torch.randn(B, T, 3 * D, device=dev) * 0.5).to(torch.bfloat16)
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    pos = (torch.randn(2 * T - 1, D, device=dev) * 0.5).to(torch.bfloat16)
    bu, bv = torch.randn(D, device=dev) * 0.1, torch.randn(D, device=dev) * 0.1
    klens = torch.tensor([max(1, T - 19 * i) for i in range(B)], device=dev, dtype=torch.int32)
    kw = dict(pos=pos, bias_u=bu, bias_v=bv, klens=klens, drop_p=p, seed=4)
    mask = ops.attn_dropmask(q, k, H, klens=klens, drop_p=p, seed=4) if p > 0 else None
    outs = {}
    for flag in (0, 2):
        # (attn_fwd_split: small launches of the per-wave kernel split the KEYS over four waves: another summation order)
        with lib.options(attn_fwd_split=0, attn_fwd4=flag):
            outs[flag] = [ops.attn_fwd(q, k, v, H, 0.125, **kw), ops.attn_fwd(q, k, v, H, 0.125, keep_mask=mask, **kw)]
            torch.cuda.synchronize()
    for (o0, l0), (o2, l2) in zip(outs[0], outs[2]):
        assert torch.equal(o0, o2) and torch.equal(l0, l2)
    assert torch.isfinite(outs[2][0][0].float()).all()


@pytest.mark.parametrize("case", ["rel", "plain", "rel_ragged"])
def test_attention_bwd_fused_vs_materialised(dev, case):
    """The single-pass backward against the materialised one on identical bf16 inputs WITH dropout (same counter-based
    mask), at a batch-like shape: several key blocks per utterance, ragged lengths, a fully masked key block."""
    from emoasr_amd import ops
    H, dk = 4, 64
    D = H * dk
    B, T, kl = {"rel": (3, 200, [200, 131, 64]), "plain": (2, 160, [160, 97]), "rel_ragged": (4, 333, [333, 300, 129, 5])}[case]
    rel = case != "plain"
    dt_ = torch.bfloat16
    klens = torch.tensor(kl, device=dev, dtype=torch.int32)
    qkv = _rnd(dev, B, T, 3 * D, dtype=dt_)
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    pos = _rnd(dev, 2 * T - 1, D, dtype=dt_) if rel else None
    bu = _rnd(dev, D, scale=0.5) if rel else None
    bv = _rnd(dev, D, scale=0.5) if rel else None
    scale = 1 / math.sqrt(dk)
    out, lse = ops.attn_fwd(q, k, v, H, scale, pos=pos, bias_u=bu, bias_v=bv, klens=klens, drop_p=0.1, seed=77)
    dout = _rnd(dev, B, T, D, dtype=dt_)
    res = {}
    from emoasr_amd import lib
    for mode in (True, "fused", "fused1"):
        with lib.options(attn_bwd_split=0 if mode == "fused1" else 1):
            dqkv = torch.full_like(qkv, float("nan"))  # every entry must be written
            dq, dk_, dv = dqkv[..., :D], dqkv[..., D:2 * D], dqkv[..., 2 * D:]
            dpos = torch.zeros(2 * T - 1, D, device=dev) if rel else None
            dbu = torch.zeros(D, device=dev) if rel else None
            dbv = torch.zeros(D, device=dev) if rel else None
            ops.attn_bwd(dout, out, lse, q, k, v, H, scale, dq, dk_, dv, pos=pos, bias_u=bu, bias_v=bv, klens=klens,
                         drop_p=0.1, seed=77, dpos=dpos, dbias_u=dbu, dbias_v=dbv, materialise="fused" if mode == "fused1" else mode)
            res[mode] = (dqkv.float(), dpos, dbu, dbv)
    a = res[True]
    for name in ("fused", "fused1"):   # the two-pass kernels (default) and the single-pass kernel
        f = res[name]
        _close(f[0][..., :D], a[0][..., :D], 3e-2, name + " dq")
        _close(f[0][..., D:2 * D], a[0][..., D:2 * D], 3e-2, name + " dk")
        _close(f[0][..., 2 * D:], a[0][..., 2 * D:], 3e-2, name + " dv")
        if rel:
            _close(f[1], a[1], 3e-2, name + " dpos")
            _close(f[2], a[2], 3e-2, name + " dbias_u")
            _close(f[3], a[3], 3e-2, name + " dbias_v")


def test_attention_bwd_fused_run_to_run(dev):
    """Race screen at a training-batch shape (both workgroup sizes): dK and dV never leave their wave's registers, so they
    must be bit-identical from run to run; dQ / dpos / dbias are sums of a few float atomics and may differ in the last bits."""
    from emoasr_amd import lib, ops
    H, dk = 4, 64
    D = H * dk
    B, T = 22, 320
    dt_ = torch.bfloat16
    kl = [T - 3 * i for i in range(B)]
    klens = torch.tensor(kl, device=dev, dtype=torch.int32)
    qkv = _rnd(dev, B, T, 3 * D, dtype=dt_)
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    pos = _rnd(dev, 2 * T - 1, D, dtype=dt_)
    bu, bv = _rnd(dev, D, scale=0.5), _rnd(dev, D, scale=0.5)
    scale = 1 / math.sqrt(dk)
    out, lse = ops.attn_fwd(q, k, v, H, scale, pos=pos, bias_u=bu, bias_v=bv, klens=klens, drop_p=0.1, seed=5)
    dout = _rnd(dev, B, T, D, dtype=dt_)
    for fw in (0, 4, 2):   # 0: the two-pass backward (default); 4 / 2: the single-pass kernel at both workgroup sizes
        with lib.options(attn_bwd_split=1 if fw == 0 else 0, attn_fw=fw):
            first = None
            for it in range(8):
                dqkv = torch.full_like(qkv, float("nan"))
                dpos = torch.zeros(2 * T - 1, D, device=dev)
                dbu, dbv = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
                ops.attn_bwd(dout, out, lse, q, k, v, H, scale, dqkv[..., :D], dqkv[..., D:2 * D], dqkv[..., 2 * D:], pos=pos,
                             bias_u=bu, bias_v=bv, klens=klens, drop_p=0.1, seed=5, dpos=dpos, dbias_u=dbu, dbias_v=dbv,
                             materialise="fused")
                cur = (dqkv.clone(), dpos, dbu, dbv)
                assert torch.isfinite(cur[0].float()).all()
                if first is None:
                    first = cur
                    continue
                assert torch.equal(cur[0][..., D:], first[0][..., D:]), f"dK/dV differ between runs (fw={fw}, run {it})"
                if fw == 0:   # dQ has one writer per row in the two-pass backward: bit-identical as well
                    assert torch.equal(cur[0][..., :D], first[0][..., :D]), f"dQ differs between runs (two-pass, run {it})"
                _close(cur[0][..., :D], first[0][..., :D], 1e-2, "dq run to run")
                _close(cur[1], first[1], 1e-3, "dpos run to run")
                _close(cur[2], first[2], 1e-3, "dbias_u run to run")


def test_gemm_nt_lse_is_the_product_plus_the_row_pass(dev):
    """emoasr_gemm_nt_lse (the CTC head in one pass over the logits: soft-max partials out of the product's epilogue) against
    emoasr_gemm_nt + a torch log-sum-exp of the STORED rows: logits bit-identical, lse to 2e-6 relative (the partials are taken
    of the values as rounded to bf16, so exp(z - lse) of a stored row sums to one), ragged M and a vocabulary that is not a
    multiple of the 256-column tile"""
    from emoasr_amd import ops
    torch.manual_seed(3)
    for M, N, K in [(4099, 10000, 256), (2500, 1000, 512)]:
        a = _rnd(dev, M, K, dtype=torch.bfloat16)
        w = (_rnd(dev, N, K) * 0.2).to(torch.bfloat16)
        bias = _rnd(dev, N)
        with ops.stream_scope():
            want = ops.gemm_nt(a, w, bias=bias)
            got, lse = ops.gemm_nt_lse(a, w, bias)
        assert torch.equal(got, want), (M, N, K)
        ref = torch.logsumexp(got.float(), -1)
        err = ((lse - ref).abs() / ref.abs().clamp(min=1)).max().item()
        assert err < 2e-6, (M, N, K, err)
        assert abs(torch.exp(got.float() - lse[:, None]).sum(-1) - 1).max().item() < 1e-4


# ---------------------------------------------------------------- conv module
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_glu(dev, dtype):
    from emoasr_amd import ops
    x = _rnd(dev, 301, 512, dtype=dtype)
    xr = x.float().requires_grad_(True)
    yr = F.glu(xr, -1)
    dy = _rnd(dev, 301, 256, dtype=dtype)
    yr.backward(dy.float())
    _close(ops.glu_fwd(x), yr, _tol(dtype, 1e-5, 1e-2), "glu")
    _close(ops.glu_bwd(x, dy), xr.grad, _tol(dtype, 1e-5, 1e-2), "glu bwd")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("T", [75, 32, 7])
def test_dwconv(dev, dtype, T):
    from emoasr_amd import ops
    B, C, K = 3, 256, 31
    x = _rnd(dev, B, T, C, dtype=dtype)
    w, b = _rnd(dev, C, K, scale=0.2), _rnd(dev, C, scale=0.1)
    xr, wr, br = x.float().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.conv1d(xr.transpose(1, 2), wr.unsqueeze(1), br, padding=15, groups=C).transpose(1, 2)
    dy = _rnd(dev, B, T, C, dtype=dtype)
    yr.backward(dy.float())
    _close(ops.dwconv_fwd(x, w, b), yr, _tol(dtype, 1e-5, 1e-2), "dwconv")
    _close(ops.dwconv_bwd_x(dy, w), xr.grad, _tol(dtype, 1e-5, 1e-2), "dwconv dx")
    dw, db = torch.empty(C, K, device=dev), torch.empty(C, device=dev)
    ops.dwconv_bwd_w(dy, x, dw, db)
    _close(dw, wr.grad, 1e-4, "dwconv dw")
    _close(db, br.grad, 1e-4, "dwconv db")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_batchnorm_swish(dev, dtype):
    from emoasr_amd import ops
    M, C, eps = 901, 256, 1e-5
    y = _rnd(dev, M, C, dtype=dtype) * 1.5 + 0.3
    g, b = _rnd(dev, C) + 1, _rnd(dev, C)
    bn = torch.nn.BatchNorm1d(C).to(dev)
    with torch.no_grad():
        bn.weight.copy_(g); bn.bias.copy_(b)
    yr = y.float().requires_grad_(True)
    zr = F.silu(bn(yr))
    dz = _rnd(dev, M, C, dtype=dtype)
    zr.backward(dz.float())
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    mean, var = ops.bn_stats(y, rm, rv, 0.1)
    _close(mean, y.float().mean(0), 1e-5, "bn mean")
    _close(var, y.float().var(0, unbiased=False), 1e-5, "bn var")
    _close(rm, bn.running_mean, 1e-5, "running mean")
    _close(rv, bn.running_var, 1e-5, "running var")
    z = ops.bn_swish_fwd(y, mean, var, g, b, eps)
    _close(z, zr, _tol(dtype, 1e-5, 1e-2), "bn swish")
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    dy = ops.bn_swish_bwd(dz, y, mean, var, g, b, eps, dg, db)
    _close(dy, yr.grad, _tol(dtype, 2e-5, 2e-2), "bn dy")
    _close(dg, bn.weight.grad, 1e-4, "bn dgamma")
    _close(db, bn.bias.grad, 1e-4, "bn dbeta")


# ---------------------------------------------------------------- CTC
def _ctc_case(dev, dtype, B=4, T=60, V=50, infeasible=False):
    elens = torch.tensor([T, T - 7, T - 20, 11][:B], device=dev, dtype=torch.int32)
    ylens = torch.tensor([12, 9, 0, 5][:B], device=dev, dtype=torch.int32)
    if infeasible:
        ylens[3] = 11  # with forced repeats below -> needs > 11 frames
    Lmax = int(ylens.max())
    labels = torch.randint(1, V, (B, Lmax), device=dev, dtype=torch.int32)
    labels[0, 3] = labels[0, 2]  # repeated label
    if infeasible:
        labels[3, :] = 7
    logits = _rnd(dev, B, T, V, dtype=dtype, scale=2.0)
    return logits, labels, elens, ylens


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("infeasible", [False, True])
def test_ctc(dev, dtype, infeasible):
    from emoasr_amd import ops
    logits, labels, elens, ylens = _ctc_case(dev, dtype, infeasible=infeasible)
    B, T, V = logits.shape
    lr = logits.float().requires_grad_(True)
    ref = F.ctc_loss(lr.transpose(0, 1).log_softmax(2), labels.long(), elens.long(), ylens.long(), blank=0,
                     reduction="sum", zero_infinity=True) / B
    ref.backward()
    nll_ref = F.ctc_loss(lr.detach().transpose(0, 1).log_softmax(2), labels.long(), elens.long(), ylens.long(),
                         blank=0, reduction="none", zero_infinity=False)
    lse = ops.row_lse(logits.view(B * T, V))
    _close(lse, torch.logsumexp(logits.float(), -1).view(-1), 1e-5, "lse")
    lp, alpha, beta, nll = ops.ctc_forward(logits, lse, labels, elens, ylens, 0)
    fin = torch.isfinite(nll_ref)
    assert torch.equal(torch.isfinite(nll), fin), (nll, nll_ref)
    _close(nll[fin], nll_ref[fin], 1e-4, "nll")
    grad = ops.ctc_grad(logits, lse, labels, elens, ylens, 0, lp, alpha, beta, nll, 1.0 / B)
    _close(grad, lr.grad, _tol(dtype, 1e-4, 1e-2), "ctc grad")
    loss = torch.where(fin, nll, torch.zeros_like(nll)).sum() / B
    _close(loss, ref.detach(), 1e-4, "loss")


@pytest.mark.parametrize("L", [1, 31, 32, 63, 64, 90], ids=lambda v: f"L{v}")
def test_ctc_lattice_label_lengths(dev, L):
    """lattices of 3 .. 181 states (one to three waves per block) against torch's CTC loss, feasibility pattern
    included"""
    from emoasr_amd import ops
    torch.manual_seed(L)
    B, T, V = 5, 2 * L + 37, 23
    elens = torch.tensor([T, T - 1, 2 * L + 1, T - 5, max(L, 1)], device=dev, dtype=torch.int32)
    ylens = torch.tensor([L, max(L - 1, 0), L, max(L // 2, 1), max(L, 1)], device=dev, dtype=torch.int32)
    labels = torch.randint(1, V, (B, L), device=dev, dtype=torch.int32)
    if L >= 3:
        labels[0, 2] = labels[0, 1]
    logits = _rnd(dev, B, T, V, scale=2.0)
    lse = ops.row_lse(logits.view(B * T, V))
    nll_ref = F.ctc_loss(logits.transpose(0, 1).log_softmax(2), labels.long(), elens.long(), ylens.long(), blank=0,
                         reduction="none", zero_infinity=False)
    lp, alpha, beta, nll = ops.ctc_forward(logits, lse, labels, elens, ylens, 0)
    fin = torch.isfinite(nll_ref)
    assert torch.equal(torch.isfinite(nll), fin), (nll, nll_ref)
    _close(nll[fin], nll_ref[fin], 1e-4, "nll")
    # alpha and beta meet: for every frame, logsumexp_s(alpha + beta - lp) = -nll
    for b in range(B):
        if not bool(fin[b]):
            continue
        n, Sb = int(elens[b]), 2 * int(ylens[b]) + 1
        tot = torch.logsumexp((alpha[b, :n, :Sb] + beta[b, :n, :Sb] - lp[b, :n, :Sb]).nan_to_num(nan=-float("inf")), -1)
        assert (tot + nll[b]).abs().max() < 2e-3 * max(1.0, float(nll[b])), (b, (tot + nll[b]).abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_ctc_greedy(dev, dtype):
    from itertools import groupby
    from emoasr_amd import ops
    B, T, V = 3, 40, 33
    logits = _rnd(dev, B, T, V, dtype=dtype)
    logits[0, 5] = logits[0, 4]  # forced repeat
    logits[1, :, 0] += 2.0       # lots of blanks
    logits[2, 3, 10] = logits[2, 3, 20] = 50.0  # tie -> first index wins
    elens = torch.tensor([40, 25, 8], device=dev, dtype=torch.int32)
    best, hyp, hyplen = ops.ctc_greedy(logits, elens, 0)
    ref_best = logits.float().argmax(-1)
    for b in range(B):
        n = int(elens[b])
        assert torch.equal(best[b, :n].long(), ref_best[b, :n]), f"argmax row {b}"
        idx = ref_best[b, :n].tolist()
        want = [x for x, _ in groupby(idx) if x != 0]
        got = hyp[b, :int(hyplen[b])].tolist()
        assert got == want, (b, got, want)
    assert int(best[2, 3]) == 10


# ---------------------------------------------------------------- optimizer / misc
def test_adam_and_norm(dev):
    from emoasr_amd import ops
    n = 100003
    p0, g = _rnd(dev, n), _rnd(dev, n)
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-3, weight_decay=1e-6)
    p, m, v = p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    nsq = torch.zeros(1, device=dev)
    for step in range(1, 4):
        gs = g * step
        pr.grad = gs.clone()
        torch.nn.utils.clip_grad_norm_([pr], 5.0)
        opt.step()
        nsq.zero_()
        ops.sqnorm(gs, nsq)
        _close(nsq, (gs.double() ** 2).sum().float().view(1), 1e-5, "sqnorm")
        ops.adam_step(p, gs, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-6, step, gnorm_sq=nsq, clip=5.0)
        _close(p, pr.detach(), 1e-5, f"adam step {step}")
    # NaN gradient norm -> step skipped
    before = p.clone()
    nsq.fill_(float("nan"))
    ops.adam_step(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-6, 4, gnorm_sq=nsq, clip=5.0)
    assert torch.equal(before, p)


def test_strided_copy_posenc(dev):
    from emoasr_amd import ops
    w = _rnd(dev, 16, 24, 3, 3)
    out = ops.strided_copy(w.permute(0, 2, 3, 1), out_dtype=torch.bfloat16)
    assert torch.equal(out, w.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16))
    acc = torch.ones(24, 16, device=dev)
    ops.strided_copy(_rnd(dev, 16, 24).t(), out=acc, accumulate=True)
    x = _rnd(dev, 2, 9, 64)
    pe = _rnd(dev, 20, 64)
    _close(ops.posenc(x, pe, 8.0), x * 8.0 + pe[:9], 1e-6, "posenc")
    _close(ops.posenc(x, None, 8.0), x * 8.0, 1e-6, "posenc scale only")
    _close(ops.add(x, x), 2 * x, 1e-6, "add")


def test_specaug_cmvn(dev):
    from emoasr_amd import ops
    B, T, Fd = 2, 50, 80
    x = _rnd(dev, B, T, Fd)
    spans = torch.tensor([[[3, 10], [70, 75], [5, 9], [0, 0]], [[0, 1], [20, 20], [40, 60], [10, 12]]],
                         device=dev, dtype=torch.int32)
    xlens = torch.tensor([50, 45], device=dev, dtype=torch.int32)
    ref = x.clone()
    for b in range(B):
        n = int(xlens[b])
        for m in range(2):
            s, e = spans[b, m].tolist()
            ref[b, :n, s:e] = 0
        for m in range(2, 4):
            s, e = spans[b, m].tolist()
            ref[b, s:min(e, n)] = 0
    got = ops.specaug_apply(x.clone(), spans, 2, 2, xlens)
    assert torch.equal(got, ref)
    mean, std = _rnd(dev, Fd), _rnd(dev, Fd).abs() + 0.5
    _close(ops.cmvn(x.clone(), mean, std), (x - mean) / std, 1e-6, "cmvn")


@pytest.mark.parametrize("zero", [True, False], ids=["zero", "mean"])
def test_adaptive_specaug_on_device(dev, zero):
    """data.SpecAugment (adaptive variant: up to 20 time bands per utterance) on a padded batch == its bands applied with
    numpy slicing, asr/spec_augment.py:39-95"""
    import random
    from types import SimpleNamespace

    import numpy as np
    from emoasr_amd.data import SpecAugment
    P = SimpleNamespace(max_mask_freq=30, num_masks_freq=2, max_mask_time_ratio=0.05, num_masks_time_ratio=0.01,
                        replace_with_zero=zero)
    xlens = [900, 640, 333]
    x = _rnd(dev, 3, 900, 80) + 0.3
    for b, n in enumerate(xlens):
        x[b, n:] = 0
    bands = SpecAugment(P, np_rng=np.random.RandomState(7), py_rng=random.Random(7)).spans(xlens, 80)
    got = SpecAugment(P, np_rng=np.random.RandomState(7), py_rng=random.Random(7))(x.clone(), xlens)
    ref = x.clone()
    for b, n in enumerate(xlens):
        fill = 0.0 if zero else x[b, :n].mean().item()
        for m, (lo, hi) in enumerate(bands[b]):
            if m < 2:
                ref[b, :n, lo:hi] = fill
            else:
                ref[b, lo:min(hi, n)] = fill
    assert (bands[:, 2:, 1] > bands[:, 2:, 0]).sum() >= 12
    _close(got, ref, 1e-6, "adaptive specaug")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_gemm_tn_grouped(dev, dtype, tr_mode):
    """grouped weight-gradient launch == the same products one by one (f32 accumulate + colsum)"""
    from emoasr_amd import ops
    shapes = [(200, 64, 96), (1000, 256, 64), (77, 40, 8), (513, 128, 256), (300, 768, 64)]
    probs, refs = [], []
    for i, (K, N1, N2) in enumerate(shapes * 4):  # 20 problems: crosses the 16-problem chunk limit
        lda = (N1 + 7) // 8 * 8
        a = _rnd(dev, K, lda, dtype=dtype)[:, :N1]
        b = _rnd(dev, K, N2, dtype=dtype, scale=K ** -0.5)
        out = torch.randn(N1, N2, device=dev)
        cs = torch.randn(N1, device=dev) if i % 2 == 0 else None
        alpha = 0.5 + 0.25 * (i % 3)
        refs.append((out + alpha * (a.float().t() @ b.float()), None if cs is None else cs + 2.0 * a.float().sum(0)))
        probs.append((a, b, out, alpha, cs, 2.0))
    ops.gemm_tn_grouped(probs)
    for i, ((a, b, out, alpha, cs, _), (ref, ref_cs)) in enumerate(zip(probs, refs)):
        _close(out, ref, _tol(dtype), f"grouped problem {i}")
        if cs is not None:
            _close(cs, ref_cs, 1e-4, f"grouped colsum {i}")


@pytest.mark.parametrize("place", [0, 1], ids=["contiguous", "placed"])
def test_gemm_tn_grouped_layer_shapes(dev, place):
    """the products of one encoder layer's backward (every N >= 128: the 128 x 128, BK = 32 tile; bias sums dealt round-robin to the
    blocks of a tile row; k slices either in contiguous eighths of the block list or dealt whole to the XCDs, option tn_place)
    against torch, with a short reduction among long ones and one product without bias sums, as csrc/layer.hip groups them"""
    from emoasr_amd import lib, ops
    K, R = 3001, 411
    shapes = [(256, 1024, K, 1), (1024, 256, K, 1), (256, 256, K, 1), (512, 256, K, 1), (256, 256, K, 1), (256, 256, R, 0),
              (768, 256, K, 1), (256, 1024, K, 1), (1024, 256, K, 1)]
    probs, refs = [], []
    for i, (n1, n2, k, cs_on) in enumerate(shapes):
        a = _rnd(dev, k, n1, dtype=torch.bfloat16)
        b = _rnd(dev, k, n2, dtype=torch.bfloat16, scale=k ** -0.5)
        out = torch.randn(n1, n2, device=dev)
        cs = torch.randn(n1, device=dev) if cs_on else None
        alpha = 1.0 if i % 2 else 0.5
        refs.append((out + alpha * (a.float().t() @ b.float()), None if cs is None else cs + alpha * a.float().sum(0)))
        probs.append((a, b, out, alpha, cs, alpha))
    with lib.options(tn_place=place):
        ops.gemm_tn_grouped(probs)
    for i, ((a, b, out, alpha, cs, _), (ref, ref_cs)) in enumerate(zip(probs, refs)):
        _close(out, ref, _tol(torch.bfloat16), f"layer product {i}")
        if cs is not None:
            _close(cs, ref_cs, 2e-3, f"layer bias sum {i}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_dwconv_bn_stats_fused(dev, dtype):
    """conv + fused batch statistics == separate conv, then torch mean / var over all B*T rows
    (padded frames included, as the reference's BatchNorm1d sees them)"""
    from emoasr_amd import ops
    for B, T, C, K in [(3, 77, 256, 31), (2, 32, 64, 15), (1, 5, 320, 31)]:
        x = _rnd(dev, B, T, C, dtype=dtype)
        w, bias = torch.randn(C, K, device=dev) * 0.2, torch.randn(C, device=dev)
        rm, rv = torch.randn(C, device=dev), torch.rand(C, device=dev) + 0.5
        nbt = torch.tensor(7, device=dev, dtype=torch.int64)
        rm0, rv0 = rm.clone(), rv.clone()
        y, mean, var = ops.dwconv_bn_stats_fwd(x, w, bias, rm, rv, 0.1, nbt)
        y_ref = ops.dwconv_fwd(x, w, bias)
        assert torch.equal(y, y_ref)
        yf = y.float().view(B * T, C)
        _close(mean, yf.mean(0), 1e-5, "fused bn mean")
        _close(var, yf.var(0, unbiased=False), 1e-4, "fused bn var")
        _close(rm, 0.9 * rm0 + 0.1 * yf.mean(0), 1e-5, "running mean")
        _close(rv, 0.9 * rv0 + 0.1 * yf.var(0, unbiased=True), 1e-4, "running var")
        assert int(nbt) == 8


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_layernorm_bwd_branch_and_deferred(dev, dtype):
    """extended LayerNorm backward: the fused branch output equals scale_dropout of the stored dx bit for
    bit, and the deferred grouped finalize gives the same dgamma / dbeta as the immediate one"""
    from emoasr_amd import ops
    M, N = 333, 256
    x, dy, dres = _rnd(dev, M, N, dtype=dtype), _rnd(dev, M, N, dtype=dtype), _rnd(dev, M, N, dtype=dtype)
    gamma = torch.randn(N, device=dev)
    mean = x.float().mean(1)
    rstd = (x.float().var(1, unbiased=False) + 1e-5).rsqrt()
    dg0, db0 = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    dx0 = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres, dg0, db0)
    deferred = []
    dg1, db1 = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    dg2, db2 = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    dx1, dyb = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres, dg1, db1, branch=(0.5, 0.1, 77), deferred=deferred)
    dx2 = ops.layernorm_bwd(dy, x, gamma, mean, rstd, None, dg2, db2, deferred=deferred)
    assert torch.equal(dx0, dx1)
    assert torch.equal(dyb, ops.scale_dropout(dx0, 0.5, 0.1, 77))
    assert float(dg1.abs().max()) == 0.0 and len(deferred) == 2  # nothing folded yet
    ops.layernorm_bwd_finalize(deferred)
    _close(dg1, dg0, 1e-5, "deferred dgamma")
    _close(db1, db0, 1e-5, "deferred dbeta")
    _close(dg2, dg0, 1e-5, "second deferred item")
    assert deferred == [] and dx2.shape == dx0.shape


@pytest.mark.parametrize("M,N,K", [(10, 768, 256), (10, 256, 1024), (1, 10000, 256), (16, 1024, 256), (7, 40, 64)])
def test_rowlin_small_m_linear(dev, M, N, K):
    """csrc/rowlin.hip: linear layers of the cached decode steps with the LayerNorms folded in, against torch"""
    from emoasr_amd import ops
    bf = torch.bfloat16
    x = _rnd(dev, M, K, dtype=bf)
    w = _rnd(dev, N, K, dtype=bf, scale=K ** -0.5)
    b = _rnd(dev, N, scale=0.3)
    ga, ba = 1 + 0.1 * _rnd(dev, K), 0.1 * _rnd(dev, K)
    gr, br = 1 + 0.1 * _rnd(dev, N), 0.1 * _rnd(dev, N)
    res = _rnd(dev, M, N, dtype=bf)
    xf, wf = x.float(), w.float()
    ln = lambda t, g, bb: F.layer_norm(t, t.shape[-1:], g, bb, 1e-12)
    _close(ops.rowlin(x, w, b), xf @ wf.t() + b, 1.5e-2, "plain")
    _close(ops.rowlin(x, w, b, act=ops.ACT_RELU, res=res), F.relu(xf @ wf.t() + b) + res.float(), 1.5e-2, "relu + residual")
    h = ln(xf, ga, ba).to(bf).float()
    _close(ops.rowlin(x, w, b, act=ops.ACT_GELU, ln_a=(ga, ba)), F.gelu(h @ wf.t() + b), 1.5e-2, "LN prologue + gelu")
    if N <= 1024:
        want = xf @ wf.t() + b + ln(res.float(), gr, br).to(bf).float()
        _close(ops.rowlin(x, w, b, res=res, ln_r=(gr, br)), want, 1.5e-2, "residual = LayerNorm(res)")
    _close(ops.rowlin(x, w, None, ln_a=(ga, ba), out_f32=True), h @ wf.t(), 1.5e-2, "f32 out")


@pytest.mark.parametrize("pos", [0, 5, 40, 63])
def test_attn_step_single_query_with_cache_append(dev, pos):
    from emoasr_amd import ops
    bf = torch.bfloat16
    nb, d, H, Lmax = 10, 256, 4, 64
    qkv = _rnd(dev, nb, 3 * d, dtype=bf)
    kc, vc = _rnd(dev, nb, Lmax, d, dtype=bf), _rnd(dev, nb, Lmax, d, dtype=bf)
    kc0, vc0 = kc.clone(), vc.clone()
    p = torch.tensor([pos], device=dev, dtype=torch.int32)
    out = ops.attn_step(qkv, kc, vc, p, H)
    assert torch.equal(kc[:, pos], qkv[:, d:2 * d]) and torch.equal(vc[:, pos], qkv[:, 2 * d:])
    keep = torch.ones(Lmax, dtype=torch.bool, device=dev)
    keep[pos] = False
    assert torch.equal(kc[:, keep], kc0[:, keep]) and torch.equal(vc[:, keep], vc0[:, keep])
    q = qkv[:, :d].float().view(nb, H, 1, d // H)
    k = kc[:, :pos + 1].float().view(nb, pos + 1, H, d // H).transpose(1, 2)
    v = vc[:, :pos + 1].float().view(nb, pos + 1, H, d // H).transpose(1, 2)
    ref = (torch.softmax(q @ k.transpose(-1, -2) / (d // H) ** 0.5, -1) @ v).transpose(1, 2).reshape(nb, d)
    _close(out, ref, 1.5e-2, "attn_step")


@pytest.mark.parametrize("V,k,use_lm", [(10000, 15, True), (10000, 15, False), (40, 6, True), (20000, 15, True), (10000, 40, True),
                                        (5000, 1, True)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_beam_scores_topk(dev, dtype, V, k, use_lm):
    """log-softmax(decoder row) + mu * log-softmax(LM row) + top-k (csrc/decoder.hip): the register-resident two-level selection,
    its LDS fallbacks (rows longer than 16 K, more than 32 candidates), and the tie rule (lowest index first)"""
    from emoasr_amd import lib, ops
    M, mu = 7, 0.3
    dec = _rnd(dev, M, V, dtype=dtype, scale=3.0)
    dec[:, 5] = dec[:, 3]                      # exact ties inside a row
    dec[2, :] = 0.0                            # a whole row of ties: indices 0 .. k - 1 in order
    lm = _rnd(dev, M, V, scale=2.0)
    lm[:, 5] = lm[:, 3]
    lm[2, :] = 0.0
    vals = torch.empty(M, k, device=dev)
    idx = torch.empty(M, k, device=dev, dtype=torch.int32)
    at = torch.empty(M, k, device=dev)
    lib.call("emoasr_beam_scores_topk", ops.dt(dec), M, V, k, dec.data_ptr(), V, lm.data_ptr() if use_lm else None, V, mu,
             vals.data_ptr(), idx.data_ptr(), at.data_ptr(), ops._stream())
    s = torch.log_softmax(dec.float(), -1)
    llm = torch.log_softmax(lm, -1)
    if use_lm:
        s = s + mu * llm
    # reference order: value descending, index ascending among equals (a stable sort of the negated scores)
    order = torch.sort(-s, dim=-1, stable=True).indices[:, :k]
    ref = torch.gather(s, 1, order)
    _close(vals, ref, 1e-5, "vals")
    got = torch.gather(s, 1, idx.long())
    _close(got, ref, 1e-5, "scores at the returned indices")
    assert (idx[2].cpu() == torch.arange(k, dtype=torch.int32)).all(), idx[2]
    for m in range(M):                          # no duplicates
        assert len(set(idx[m].tolist())) == k
    if use_lm:
        _close(at, torch.gather(llm, 1, idx.long()), 1e-5, "lm_at")


@pytest.mark.parametrize("U,B,H,with_state", [(9, 36, 512, False), (5, 50, 512, True), (7, 4, 128, False), (3, 17, 256, True)])
def test_lstm_seq_cooperative_matches_the_step_chain(dev, U, B, H, with_state):
    """csrc/lstm_coop.hip (one cooperative launch for the whole recurrence of a layer) against the per-position chain
    gemm_nt + lstm_cell_fwd: same h / c / activated gates to bf16 rounding"""
    from emoasr_amd import ops
    dt_ = torch.bfloat16
    pre = _rnd(dev, U, B, 4 * H, dtype=dt_, scale=1.0)
    w_hh = _rnd(dev, 4 * H, H, dtype=dt_, scale=H ** -0.5)
    h0 = _rnd(dev, B, H, dtype=dt_, scale=0.5) if with_state else None
    c0 = _rnd(dev, B, H, scale=0.5) if with_state else None
    assert ops.lstm_seq_supported(pre, B, H)
    hseq = torch.empty(U, B, H, device=dev, dtype=dt_)
    cseq = torch.empty(U, B, H, device=dev)
    gact = torch.empty(U, B, 4 * H, device=dev, dtype=dt_)
    ops.lstm_seq_fwd(pre, w_hh, h0, c0, hseq, cseq, gact)
    h_ref = torch.empty_like(hseq); c_ref = torch.empty_like(cseq); g_ref = torch.empty_like(gact)
    hp, cp = h0, c0
    for u in range(U):
        gates = pre[u] if hp is None else ops.gemm_nt(hp, w_hh, residual=pre[u], res_scale=1.0)
        ops.lstm_cell_fwd(gates, cp, h_ref[u], c_ref[u], g_ref[u])
        hp, cp = h_ref[u], c_ref[u]
    torch.cuda.synchronize()
    _close(hseq, h_ref, 3e-2, "hseq")
    _close(cseq, c_ref, 3e-2, "cseq")
    _close(gact, g_ref, 3e-2, "gact")


def test_lstm_seq_cooperative_survives_changing_grid_sizes(dev):
    """The grid barrier's base is tracked by the host per launch (csrc/lstm_coop.hip: lstm_base), so launches whose workgroup
    counts G = H / 16 differ may follow each other in any order: H = 128 with U = 4 leaves the shared counter at 24, which is
    not a multiple of the next launch's G = 32 (the round-2 kernels derived the base as counter - counter % G and released the
    first barrier of that launch after 8 of 32 arrivals); H = 320 gives a G that is not a power of two."""
    from emoasr_amd import lib, ops
    dt_ = torch.bfloat16

    def run(U, B, H):
        pre = _rnd(dev, U, B, 4 * H, dtype=dt_, scale=1.0)
        w_hh = _rnd(dev, 4 * H, H, dtype=dt_, scale=H ** -0.5)
        hseq = torch.empty(U, B, H, device=dev, dtype=dt_)
        cseq = torch.empty(U, B, H, device=dev)
        gact = torch.empty(U, B, 4 * H, device=dev, dtype=dt_)
        ops.lstm_seq_fwd(pre, w_hh, None, None, hseq, cseq, gact)
        h_ref = torch.empty_like(hseq); c_ref = torch.empty_like(cseq); g_ref = torch.empty_like(gact)
        hp, cp = None, None
        for u in range(U):
            gates = pre[u] if hp is None else ops.gemm_nt(hp, w_hh, residual=pre[u], res_scale=1.0)
            ops.lstm_cell_fwd(gates, cp, h_ref[u], c_ref[u], g_ref[u])
            hp, cp = h_ref[u], c_ref[u]
        torch.cuda.synchronize()
        _close(hseq, h_ref, 3e-2, f"hseq H={H} U={U}")
        # backward on the same shapes
        dh_seq = _rnd(dev, U, B, H, dtype=dt_, scale=0.5)
        dgp = torch.empty(U, B, 4 * H, device=dev, dtype=dt_)
        ops.lstm_seq_bwd(dh_seq, gact, cseq, None, w_hh, dgp)
        assert torch.isfinite(dgp.float()).all()

    for U, B, H in [(4, 36, 128), (9, 36, 512), (6, 20, 320), (3, 36, 512), (5, 8, 96), (7, 36, 512)]:
        run(U, B, H)
        assert lib.size_query("emoasr_lstm_coop_status") == 0, (U, B, H)


@pytest.mark.parametrize("U,B,H", [(7, 150, 512), (5, 65, 256), (4, 128, 512), (6, 500, 128)])
def test_lstm_seq_groups_of_64_sequences_in_one_launch(dev, U, B, H):
    """more than 64 sequences (the prediction network of several stacked micro-batches): ceil(B / 64) groups of H / 16 workgroups
    in ONE launch, each with its own barrier counter -- bit-identical, forward and backward, to one launch per 64-row slab"""
    from emoasr_amd import lib, ops
    dt_ = torch.bfloat16
    pre = _rnd(dev, U, B, 4 * H, dtype=dt_, scale=1.0)
    w_hh = _rnd(dev, 4 * H, H, dtype=dt_, scale=H ** -0.5)
    h0, c0 = _rnd(dev, B, H, dtype=dt_, scale=0.5), _rnd(dev, B, H, scale=0.5)
    dh_seq = _rnd(dev, U, B, H, dtype=dt_, scale=0.5)
    assert ops.lstm_seq_supported(pre, B, H)
    hseq, cseq = torch.empty(U, B, H, device=dev, dtype=dt_), torch.empty(U, B, H, device=dev)
    gact, dgp = torch.empty(U, B, 4 * H, device=dev, dtype=dt_), torch.empty(U, B, 4 * H, device=dev, dtype=dt_)
    ops.lstm_seq_fwd(pre, w_hh, h0, c0, hseq, cseq, gact)
    ops.lstm_seq_bwd(dh_seq, gact, cseq, c0, w_hh, dgp)
    assert lib.size_query("emoasr_lstm_coop_status") == 0
    for b0 in range(0, B, 64):
        b1 = min(B, b0 + 64)
        n = b1 - b0
        hs, cs = torch.empty(U, n, H, device=dev, dtype=dt_), torch.empty(U, n, H, device=dev)
        ga, dg = torch.empty(U, n, 4 * H, device=dev, dtype=dt_), torch.empty(U, n, 4 * H, device=dev, dtype=dt_)
        ops.lstm_seq_fwd(pre[:, b0:b1].contiguous(), w_hh, h0[b0:b1].contiguous(), c0[b0:b1].contiguous(), hs, cs, ga)
        ops.lstm_seq_bwd(dh_seq[:, b0:b1].contiguous(), ga, cs, c0[b0:b1].contiguous(), w_hh, dg)
        assert torch.equal(hs, hseq[:, b0:b1]) and torch.equal(cs, cseq[:, b0:b1]) and torch.equal(ga, gact[:, b0:b1]), (b0, "forward")
        assert torch.equal(dg, dgp[:, b0:b1]), (b0, "backward")
    assert lib.size_query("emoasr_lstm_coop_status") == 0


@pytest.mark.parametrize("U,B,H,with_c0", [(9, 36, 512, False), (5, 50, 512, True), (7, 4, 128, False), (3, 17, 256, True)])
def test_lstm_seq_backward_cooperative_matches_the_step_chain(dev, U, B, H, with_c0):
    """the backward recurrence of csrc/lstm_coop.hip against the per-position chain lstm_cell_bwd + gemm_nn"""
    from emoasr_amd import lib, ops
    dt_ = torch.bfloat16
    gact = torch.sigmoid(_rnd(dev, U, B, 4 * H)).to(dt_)
    gact[:, :, 2 * H:3 * H] = torch.tanh(_rnd(dev, U, B, H)).to(dt_)
    cseq = _rnd(dev, U, B, H, scale=0.7)
    c0 = _rnd(dev, B, H, scale=0.7) if with_c0 else None
    dh_seq = _rnd(dev, U, B, H, dtype=dt_, scale=0.5)
    w_hh = _rnd(dev, 4 * H, H, dtype=dt_, scale=H ** -0.5)
    dgp = torch.empty(U, B, 4 * H, device=dev, dtype=dt_)
    ops.lstm_seq_bwd(dh_seq, gact, cseq, c0, w_hh, dgp)
    assert lib.size_query("emoasr_lstm_coop_status") == 0
    ref = torch.empty_like(dgp)
    dc = torch.zeros(B, H, device=dev)
    dh_rec = None
    for u in reversed(range(U)):
        ops.lstm_cell_bwd(dh_seq[u], dh_rec, dc, gact[u], cseq[u - 1] if u > 0 else c0, cseq[u], ref[u])
        if u > 0:
            dh_rec = ops.gemm_nn(ref[u], w_hh)
    torch.cuda.synchronize()
    _close(dgp, ref, 3e-2, "dgp")


