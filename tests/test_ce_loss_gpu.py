"""The cross-entropy side at kernel level: lsm_loss, embed_fwd / embed_bwd (csrc/decoder.hip) and soft_ce (csrc/distill.hip) against
the float64 references of tests/ctc_ref.py (pinned on the CPU by tests/test_ctc_ref_cpu.py): vocabularies of less than one,
exactly one, one + 1 and many trips of the 256-thread stride, labels on the first and last column, strided rows, zero-weight rows,
soft rows that are no distributions, row lists, the second trip of the embedding's 4096-block grid-stride loop, the dropout mask.

Bounds (none taken from the kernels under test):
  loss rows        |got - ref64| <= max(4 * e32, (ceil(V / 256) + 10) * 2^-24 * A): e32 = the error of the float32 evaluation of the
                   same formulas (dtype=float32 of the references, libm accuracy) on the same case; A = the float64 sum of the
                   magnitudes of the terms w * q[v] * log p[v] the row is the sum of -- the worst-case rounding of a 256-thread
                   strided sum (ceil(V / 256) additions per thread) followed by the wave and block reductions (6 + 4 levels)
  gradients        4 * e32; bf16: + 2^-8 |ref|, one ulp of output rounding
  embed_fwd        exact: bf16 / f32((table * scale) + pe) is two correctly rounded f32 operations and one cast (no contraction)
  embed_bwd        n * 2^-24 * sum |terms| per table entry with n contributions, the terms being the f32 products the kernel
                   adds: only the order of the atomics is free
  masks, zero rows, untouched rows   exact

MEASURED on an MI355X, worst share of the bound: lsm_loss loss 0.25, gradient 0.96 (bf16 output rounding; f32 0.37); soft_ce loss
0.26, gradient 0.96 (bf16; f32 0.70); embed_bwd 0.50; kept share of the dropout mask on 1 184 256 elements 0.70028 (+0.67 sd)."""
import math

import numpy as np
import pytest
import torch

from tests.ctc_ref import lsm_ref, soft_ce_ref

pytestmark = pytest.mark.gpu

P24, P8 = 2.0 ** -24, 2.0 ** -8
NAN = float("nan")
_DT = [torch.float32, torch.bfloat16]
_DT_IDS = ["f32", "bf16"]
_VOCABS = [2, 3, 255, 256, 257, 1000, 10000]
_EPS = [0.0, float(np.float32(0.1))]     # (what the kernels receive: the smoothing weight is a C float)
_EPS_IDS = ["eps0", "eps0.1"]


def _i32(a, dev):
    return torch.as_tensor(np.asarray(a)).to(torch.int32).to(dev)


def _f32(a, dev):
    return torch.as_tensor(np.asarray(a, np.float32)).to(dev)


def _worst(got, ref, bound):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), "non-finite value"
    err = np.abs(got - ref)
    return float(err.max()), float((err / (np.broadcast_to(bound, ref.shape) + 1e-300)).max())


def _report(name, ref, m32, loss, grad, V, dtype):
    """loss rows and gradient of one call against the reference; -> nothing, asserts"""
    lines = []
    e32 = float(np.abs(m32.loss.astype(np.float64) - ref.loss).max())
    err, ratio = _worst(loss, ref.loss, np.maximum(4 * e32, (math.ceil(V / 256) + 10) * P24 * ref.mag))
    lines.append(("loss", err, e32, ratio))
    e32 = float(np.abs(m32.grad.astype(np.float64) - ref.grad).max())
    bound = 4 * e32 + (P8 * np.abs(ref.grad) if dtype == torch.bfloat16 else 0.0)
    err, ratio = _worst(grad, ref.grad, bound)
    lines.append(("grad", err, e32, ratio))
    print(f"[measured] {name}: " + ", ".join(f"{k} err {e:.2e} (f32 model {m:.2e}) {r:.2f} of bound" for k, e, m, r in lines))
    for k, e, m, r in lines:
        assert r <= 1.0, (name, k, e, m, r)


def _strided(z, dev, pad=5):
    """z [M,V] on the device as the [:, :V] view of a NaN-filled [M, V + pad] buffer"""
    M, V = z.shape
    wide = torch.full((M, V + pad), NAN, dtype=z.dtype)
    wide[:, :V] = z
    return wide.to(dev)[:, :V]


# ---- lsm_loss ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", _EPS, ids=_EPS_IDS)
@pytest.mark.parametrize("V", _VOCABS)
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_lsm_loss(dev, dtype, V, eps):
    """five rows of a strided logits view: labels on column 0 and on the last column, one row of weight 0 (loss 0, zero gradient
    row), gscale * gscale_dev"""
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(V)
    M = 5
    z = (torch.randn(M, V, generator=g) * 2).to(dtype)
    labels = [0, V - 1, int(torch.randint(0, V, (1,), generator=g)), V - 1, 0]
    w = [0.5, 1.0, 0.0, 0.25, 2.0]
    gs, gdev = 0.5, 0.25
    z64 = z.double().numpy()
    ref = lsm_ref(z64, labels, w, eps, gs=gs * gdev)
    m32 = lsm_ref(z64, labels, w, eps, gs=gs * gdev, dtype=np.float32)
    zd = _strided(z, dev)
    assert zd.stride(0) == V + 5
    loss, grad = ops.lsm_loss(zd, _i32(labels, dev), _f32(w, dev), eps, want_grad=True, gscale=gs,
                              gscale_dev=torch.tensor([gdev], device=dev))
    loss, grad = loss.cpu().numpy(), grad.float().cpu().numpy()
    _report(f"lsm_loss V={V} eps={eps:.1f} {_DT_IDS[_DT.index(dtype)]}", ref, m32, loss, grad, V, dtype)
    assert loss[2] == 0.0 and (grad[2] == 0).all()
    # the same product passed on the host: the same bits
    loss2, grad2 = ops.lsm_loss(zd, _i32(labels, dev), _f32(w, dev), eps, want_grad=True, gscale=gs * gdev)
    assert np.array_equal(loss2.cpu().numpy(), loss) and np.array_equal(grad2.float().cpu().numpy(), grad)
    loss3, none = ops.lsm_loss(zd, _i32(labels, dev), _f32(w, dev), eps)
    assert none is None and np.array_equal(loss3.cpu().numpy(), loss)


# ---- soft_ce -------------------------------------------------------------------------------------------------------------------------
def _soft_case(dtype, V, M, g):
    z = (torch.randn(M, V, generator=g) * 2).to(dtype)
    soft = torch.rand(3, V, generator=g)
    soft[0] /= soft[0].sum()          # one distribution; row 1 sums to about V / 2, row 2 to about V / 20
    soft[2] *= 0.1
    return z, soft


@pytest.mark.parametrize("eps", _EPS, ids=_EPS_IDS)
@pytest.mark.parametrize("V", _VOCABS)
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_soft_ce(dev, dtype, V, eps):
    """six rows: soft only, hard only, both, neither (loss 0, zero gradient), both with a source row used before, soft only -- the
    sources repeated and permuted into a table of three rows, two of which do not sum to 1 (the sum(q) factor of the gradient);
    hard labels on column 0 and on the last column; strided logits and gradient rows; gscale_dev"""
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(7 * V + 1)
    R = 6
    z, soft = _soft_case(dtype, V, R, g)
    src = [2, -1, 0, -1, 2, 1]
    hard = [-1, 0, V - 1, -1, V // 2, -1]
    ws = [0.5, 9.0, 1.0, 9.0, 0.3, 2.0]
    wh = [9.0, 1.5, 0.5, 9.0, 0.7, 9.0]
    gs, gdev = 2.0, 0.25
    z64, s64 = z.double().numpy(), soft.double().numpy()
    ws32, wh32 = np.asarray(ws, np.float32).astype(np.float64), np.asarray(wh, np.float32).astype(np.float64)
    ref = soft_ce_ref(z64, s64, src, hard, ws32, wh32, eps, gs=gs * gdev)
    m32 = soft_ce_ref(z64, s64, src, hard, ws32, wh32, eps, gs=gs * gdev, dtype=np.float32)
    zd = _strided(z, dev)
    flat = torch.full((R * (V + 3) + 64,), NAN, device=dev, dtype=dtype)
    gbuf = flat[:R * (V + 3)].view(R, V + 3)[:, :V]
    loss, grad = ops.soft_ce(zd, soft.to(dev), _i32(src, dev), _i32(hard, dev), _f32(ws, dev), _f32(wh, dev), eps, want_grad=True,
                             gscale=gs, gscale_dev=torch.tensor([gdev], device=dev), grad=gbuf)
    assert grad.data_ptr() == gbuf.data_ptr()
    assert bool(torch.isnan(flat[R * (V + 3):]).all()) and bool(torch.isnan(flat[:R * (V + 3)].view(R, V + 3)[:, V:]).all())
    loss, grad = loss.cpu().numpy(), grad.float().cpu().numpy()
    _report(f"soft_ce V={V} eps={eps:.1f} {_DT_IDS[_DT.index(dtype)]}", ref, m32, loss, grad, V, dtype)
    assert loss[3] == 0.0 and (grad[3] == 0).all()


@pytest.mark.parametrize("V", [257, 1000])
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_soft_ce_row_list(dev, dtype, V):
    """lrow names 3 of 8 logits rows, out of order; the gradient buffer is zero-filled by the caller: the other rows stay exactly 0"""
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(11 * V)
    M, eps = 8, _EPS[1]
    z, soft = _soft_case(dtype, V, M, g)
    lrow, src, hard = [6, 1, 4], [1, -1, 0], [-1, V - 1, 3]
    ws, wh = [0.5, 9.0, 1.0], [9.0, 1.5, 0.5]
    z64, s64 = z.double().numpy(), soft.double().numpy()
    ref = soft_ce_ref(z64, s64, src, hard, ws, wh, eps, gs=0.5, lrow=lrow)
    m32 = soft_ce_ref(z64, s64, src, hard, ws, wh, eps, gs=0.5, lrow=lrow, dtype=np.float32)
    zd = z.to(dev)
    loss, grad = ops.soft_ce(zd, soft.to(dev), _i32(src, dev), _i32(hard, dev), _f32(ws, dev), _f32(wh, dev), eps,
                             lrow=_i32(lrow, dev), want_grad=True, gscale=0.5)
    assert loss.shape == (3,) and grad.shape == (M, V)
    loss, grad = loss.cpu().numpy(), grad.float().cpu().numpy()
    _report(f"soft_ce lrow V={V} {_DT_IDS[_DT.index(dtype)]}", ref, m32, loss, grad, V, dtype)
    assert (grad[[0, 2, 3, 5, 7]] == 0).all() and (np.abs(grad[lrow]).max(1) > 0).all()


# ---- embedding -----------------------------------------------------------------------------------------------------------------------
_EMBED = [(3, 5, 64), (2, 7, 144), (9, 257, 512)]     # the last: M * d = 1 184 256 > 4096 * 256, a second trip of the grid-stride loop
_NTAB = 11


def _ids(B, L, g, mode):
    if mode == "equal":
        return torch.full((B, L), 4, dtype=torch.int32)
    ids = torch.randint(0, _NTAB, (B, L), generator=g).to(torch.int32)
    ids[0, :2] = 7          # repeated within a row as well
    return ids


def _cast(a32, dtype):
    return torch.from_numpy(np.ascontiguousarray(a32)).to(dtype)


@pytest.mark.parametrize("ids_mode", ["repeated", "equal"])
@pytest.mark.parametrize("with_pe", [False, True], ids=["no_pe", "pe"])
@pytest.mark.parametrize("B,L,d", _EMBED)
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_embed_forward_without_dropout_is_exact(dev, dtype, B, L, d, with_pe, ids_mode):
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(B * L + d)
    table = torch.randn(_NTAB, d, generator=g).to(dtype)
    pe = torch.randn(L + 3, d, generator=g) if with_pe else None      # more rows than L: the position is m % L
    ids = _ids(B, L, g, ids_mode)
    scale = 1.7
    out = ops.embed_fwd(ids.to(dev), table.to(dev), None if pe is None else pe.to(dev), scale)
    v = table.float().numpy()[ids.long().numpy()] * np.float32(scale)      # [B,L,d] f32, one rounding
    if with_pe:
        v = v + pe.numpy()[None, :L]                                       # f32, one rounding
    assert v.dtype == np.float32
    assert out.shape == (B, L, d) and out.dtype == dtype
    assert torch.equal(out.cpu(), _cast(v, dtype))


@pytest.mark.parametrize("B,L,d", _EMBED)
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_embed_dropout_mask_and_backward(dev, dtype, B, L, d):
    """p = 0.3.  The mask, read off a forward over a table of ones: kept entries are scale * (1 / (1 - p)) in f32, rounded to the
    output type; one seed gives one mask, another seed another; on the 1.18 M-element case the kept share lies within 4.5 binomial
    standard deviations of 0.7.  The backward adds dout * scale * mask / (1 - p) into the table rows -- index_add over that mask."""
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(B * L + d + 1)
    p, scale, seed = 0.3, 1.7, 1234
    ids = _ids(B, L, g, "repeated")
    ones = torch.ones(_NTAB, d, dtype=dtype, device=dev)
    out = ops.embed_fwd(ids.to(dev), ones, None, scale, drop_p=p, seed=seed)
    again = ops.embed_fwd(ids.to(dev), ones, None, scale, drop_p=p, seed=seed)
    other = ops.embed_fwd(ids.to(dev), ones, None, scale, drop_p=p, seed=seed + 1)
    assert torch.equal(out, again)
    mask = (out != 0).cpu().numpy()
    inv = np.float32(1) / (np.float32(1) - np.float32(p))
    kept = _cast(np.asarray([np.float32(scale) * inv], np.float32), dtype)[0]
    assert bool((out[out != 0] == kept.to(dev)).all())
    mask_other = (other != 0).cpu().numpy()
    assert (mask != mask_other).mean() > 0.25          # independent masks differ on 2 * 0.7 * 0.3 = 42 % of the entries
    n = mask.size
    share = mask.mean()
    print(f"[measured] embed dropout {B}x{L}x{d}: kept share {share:.5f} of {n}, {(share - 0.7) / math.sqrt(0.21 / n):+.2f} sd")
    if n > 1 << 20:
        assert abs(share - 0.7) <= 4.5 * math.sqrt(0.21 / n)
    dout = torch.randn(B, L, d, generator=g).to(dtype)
    dtable = torch.zeros(_NTAB, d, device=dev)
    ops.embed_bwd(ids.to(dev), dout.to(dev), scale, dtable, drop_p=p, seed=seed)
    terms = (dout.float().numpy() * np.float32(scale)) * np.where(mask, inv, np.float32(0)).astype(np.float32)     # f32, as added
    assert terms.dtype == np.float32
    idn = ids.long().numpy().reshape(-1)
    ref, mag = np.zeros((_NTAB, d)), np.zeros((_NTAB, d))
    np.add.at(ref, idn, terms.reshape(-1, d).astype(np.float64))
    np.add.at(mag, idn, np.abs(terms.reshape(-1, d)).astype(np.float64))
    count = np.bincount(idn, minlength=_NTAB)[:, None]
    err, ratio = _worst(dtable.cpu().numpy(), ref, count * P24 * mag)
    print(f"[measured] embed_bwd {B}x{L}x{d} {_DT_IDS[_DT.index(dtype)]}: err {err:.2e} {ratio:.2f} of bound")
    assert ratio <= 1.0, (err, ratio)
    assert (dtable.cpu().numpy()[count[:, 0] == 0] == 0).all()


@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_embed_backward_without_dropout(dev, dtype):
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(5)
    B, L, d, scale = 3, 5, 64, 1.7
    for mode in ("repeated", "equal"):
        ids = _ids(B, L, g, mode)
        dout = torch.randn(B, L, d, generator=g).to(dtype)
        dtable = torch.zeros(_NTAB, d, device=dev)
        ops.embed_bwd(ids.to(dev), dout.to(dev), scale, dtable)
        terms = dout.float().numpy() * np.float32(scale)
        idn = ids.long().numpy().reshape(-1)
        ref, mag = np.zeros((_NTAB, d)), np.zeros((_NTAB, d))
        np.add.at(ref, idn, terms.reshape(-1, d).astype(np.float64))
        np.add.at(mag, idn, np.abs(terms.reshape(-1, d)).astype(np.float64))
        count = np.bincount(idn, minlength=_NTAB)[:, None]
        err, ratio = _worst(dtable.cpu().numpy(), ref, count * P24 * mag)
        print(f"[measured] embed_bwd p=0 {mode} {_DT_IDS[_DT.index(dtype)]}: err {err:.2e} {ratio:.2f} of bound")
        assert ratio <= 1.0, (err, ratio)
