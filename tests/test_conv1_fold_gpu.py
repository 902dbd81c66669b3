"""The first convolution's weight gradient folded into the large-tile data gradient of the second (emoasr_conv2_dgrad_w1)
against the two kernels it replaces: emoasr_conv2_dgrad_kc (dy1 written out) + emoasr_conv1_wgrad (dy1 read back)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _close(got, ref, tol, what):
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def _inputs(dev, B, T, Fd, C):
    from emoasr_amd import ops
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + T + Fd + C)
    x = torch.randn(B, T, Fd, generator=g).to(dev)
    w1 = (torch.randn(C, 9, generator=g) * 0.3).to(dev)
    b1 = (torch.randn(C, generator=g) * 0.1).to(dev)
    y1 = ops.conv1_fwd(x, w1, b1, torch.bfloat16)
    T1, F1 = y1.shape[1], y1.shape[2]
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    dy2 = torch.randn(B * T2 * F2, C, generator=g)
    dy2 = (dy2 * (torch.rand(B * T2 * F2, C, generator=g) > 0.4)).to(dev, torch.bfloat16)   # (ReLU-masked like the step's)
    wt = (torch.randn(C, 9 * C, generator=g) * (9 * C) ** -0.5).to(dev, torch.bfloat16)
    return x, y1, dy2, wt


@pytest.mark.parametrize("bm", [0, 256, 192, 128])
@pytest.mark.parametrize("B,T,Fd,C", [(3, 41, 80, 256), (2, 30, 23, 512), (5, 97, 80, 256), (1, 7, 7, 256)])
def test_conv1_wgrad_folded_into_conv2_dgrad(dev, bm, B, T, Fd, C):
    """every tile height, ragged class tiles, C = 512 (two column tiles), the smallest input; plain and accumulating calls"""
    from emoasr_amd import lib, ops
    x, y1, dy2, wt = _inputs(dev, B, T, Fd, C)
    with lib.options(big_bm=bm):
        dy1 = ops.conv2_dgrad_kc(dy2, wt, y1)
        dw_ref = torch.empty(C, 9, device=dev)
        db_ref = torch.empty(C, device=dev)
        ops.conv1_wgrad(x, dy1, dw_ref, db_ref)
        dw = torch.full((C, 9), float("nan"), device=dev)
        db = torch.full((C,), float("nan"), device=dev)
        ops.conv2_dgrad_w1(dy2, wt, y1, x, dw, db)
        _close(dw, dw_ref, 1e-4, "conv1 wgrad (folded)")
        _close(db, db_ref, 1e-4, "conv1 bgrad (folded)")
        base_w, base_b = torch.randn(C, 9, device=dev), torch.randn(C, device=dev)
        dw2, db2 = base_w.clone(), base_b.clone()
        ops.conv2_dgrad_w1(dy2, wt, y1, x, dw2, db2, accumulate=True)
        _close(dw2 - base_w, dw_ref, 1e-4, "conv1 wgrad (folded, accumulate)")
        _close(db2 - base_b, db_ref, 1e-4, "conv1 bgrad (folded, accumulate)")


def test_conv1_fold_matches_torch_autograd(dev):
    """the folded gradient of a whole Conv2d(1, C) + ReLU + Conv2d(C, C) stack against torch autograd on the same bf16 operands"""
    import torch.nn.functional as F
    from emoasr_amd import ops
    B, T, Fd, C = 2, 37, 40, 256
    g = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn(B, T, Fd, generator=g).to(dev)
    w1 = (torch.randn(C, 1, 3, 3, generator=g) * 0.3).to(dev)
    b1 = (torch.randn(C, generator=g) * 0.1).to(dev)
    w2 = (torch.randn(C, C, 3, 3, generator=g) * (9 * C) ** -0.5).to(dev, torch.bfloat16)
    y1 = ops.conv1_fwd(x, w1.reshape(C, 9).contiguous(), b1, torch.bfloat16)
    w1r, b1r = w1.clone().requires_grad_(True), b1.clone().requires_grad_(True)
    z1 = F.conv2d(x.unsqueeze(1), w1r, b1r, stride=2)
    y1f = F.relu(z1)
    z2 = F.conv2d(y1f, w2.float(), stride=2)
    T2, F2 = z2.shape[2], z2.shape[3]
    dy2 = torch.randn(B, T2, F2, C, generator=g).to(dev, torch.bfloat16)
    # the reference sees the kernel's own bf16 rounding of dy1: the data gradient in f32 of the same bf16 operands, then rounded
    y1r = y1.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.conv2d(y1r, w2.float(), stride=2).backward(dy2.float().permute(0, 3, 1, 2))
    dy1 = (y1r.grad * (y1r > 0)).to(torch.bfloat16).float()
    z1.backward(dy1)
    dw = torch.zeros(C, 9, device=dev)
    db = torch.zeros(C, device=dev)
    wt = w2.permute(1, 2, 3, 0).reshape(C, 9 * C).contiguous()
    ops.conv2_dgrad_w1(dy2.reshape(-1, C), wt, y1, x, dw, db, accumulate=True)
    _close(dw, w1r.grad.reshape(C, 9), 2e-2, "conv1 wgrad vs autograd")
    _close(db, b1r.grad, 2e-2, "conv1 bgrad vs autograd")
