"""The logit-free cross-entropy vocabulary head (ops.ce_head_fwd / ce_head_bwd: csrc/gemm_big.hip) at the LM's full size:
V = 10 000, d = 256, 4 096 rows, about 10 % of the labels ignored (-100), random bf16 operands.

The truth is float64 torch on the bf16-rounded operands.  The fused path skips one bf16 rounding of the logits, so it gets NO margin:
its per-row loss and its dz rows must be no further from the truth than the materialised path (gemm_nt_lse + lsm_loss, what the
head was before) is on the same inputs.  dX / dW are compared with gemm_nn / gemm_tn applied to the materialised gradient, measured
the same way; the peak of additional device memory over forward + backward must stay below ONE [rows, V] bf16 matrix (the
materialised path holds two: logits and their gradient)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, V, D = 4096, 10000, 256


def _inputs(dev):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(ROWS, D, generator=g).to(torch.bfloat16)
    w = (torch.randn(V, D, generator=g) * 0.15).to(torch.bfloat16)      # logits of a few units, like a trained head's
    bias = torch.randn(V, generator=g) * 0.5
    labels = torch.randint(0, V, (ROWS,), generator=g, dtype=torch.int64)
    labels[torch.rand(ROWS, generator=g) < 0.1] = -100
    valid = labels != -100
    wrow = valid.to(torch.float32) / int(valid.sum())
    return x.to(dev), w.to(dev), bias.to(dev), labels, wrow.to(dev)


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()


def test_fused_head_against_float64_and_the_materialised_path(dev):
    from emoasr_amd import ops
    x, w, bias, labels, wrow = _inputs(dev)
    lab_dev = labels.clamp(min=0).to(torch.int32).to(dev)
    lab_raw = labels.to(torch.int32).to(dev)        # the fused entry clamps ignored labels itself
    assert ops.ce_head_ok(x, w)
    # ---- truth: float64 on the bf16-rounded operands
    z = x.double() @ w.double().t() + bias.double()
    lse = torch.logsumexp(z, dim=1)
    idx = labels.clamp(min=0).to(dev)
    true_rows = wrow.double() * (lse - z.gather(1, idx[:, None])[:, 0])
    sample = torch.randperm(ROWS, generator=torch.Generator().manual_seed(5))[:64].to(dev)
    true_dz = wrow.double()[sample, None] * (torch.softmax(z[sample], dim=1) - torch.nn.functional.one_hot(idx[sample], V))
    del z
    # ---- the materialised path (the parent's head): logits + lse in one pass, loss and gradient rows from the stored logits
    logits, _ = ops.gemm_nt_lse(x, w, bias)
    mat_rows, mat_dz = ops.lsm_loss(logits, lab_dev, wrow, 0.0, True)
    mat_dw = torch.zeros(V, D, device=dev)
    mat_db = torch.zeros(V, device=dev)
    ops.gemm_tn(mat_dz, x, out=mat_dw, accumulate=True, colsum=mat_db)
    mat_dx = ops.gemm_nn(mat_dz, w)
    mat_row_err = (mat_rows.double() - true_rows).abs().max().item()
    mat_dz_err = (mat_dz[sample].double() - true_dz).abs().max().item()
    del logits
    # ---- the fused path, its peak of additional memory over forward + backward
    dw = torch.zeros(V, D, device=dev)
    db = torch.zeros(V, device=dev)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    rows, logp, ctx = ops.ce_head_fwd(x, w, bias, lab_raw, wrow)
    dx = ops.ce_head_bwd(x, w, bias, ctx, dw, db)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"fused head: peak additional memory {peak / 2**20:.1f} MiB against {ROWS * V * 2 / 2**20:.1f} MiB for one logits matrix")
    assert peak < ROWS * V * 2, (peak, ROWS * V * 2)
    fused_row_err = (rows.double() - true_rows).abs().max().item()
    # the same 64 rows of dz from the fused gradient entry (one chunk holding exactly those rows)
    lse_f, ycol, _ = ctx
    xs = x[sample].contiguous()
    sctx = (lse_f[sample].contiguous(), ycol[sample].contiguous(), wrow[sample].contiguous())
    dz_s = torch.empty(64, V, device=dev, dtype=torch.bfloat16)
    coef = torch.empty(64, 4, device=dev, dtype=torch.float32)
    from emoasr_amd import lib
    lib.call("emoasr_ce_head_grad", ops.dt(xs), 64, V, D, ops._p(xs), ops._p(w), ops._p(bias), ops._p(sctx[0]), ops._p(sctx[1]),
             ops._p(sctx[2]), 1.0, None, ops._p(coef), ops._p(dz_s), V, ops._stream())
    fused_dz_err = (dz_s.double() - true_dz).abs().max().item()
    msg = (f"per-row loss max error: fused {fused_row_err:.3e}, materialised {mat_row_err:.3e}; "
           f"dz (64 rows) max error: fused {fused_dz_err:.3e}, materialised {mat_dz_err:.3e}")
    print(msg)
    assert fused_row_err <= mat_row_err, msg
    assert fused_dz_err <= mat_dz_err, msg
    # log-probabilities of the labelled rows (what LM.score and ppl_lm read)
    valid = (labels != -100).to(dev)
    true_logp = -(true_rows / wrow.double().clamp(min=1e-30))[valid]
    assert (logp.double()[valid] - true_logp).abs().max().item() < 1e-3
    assert not rows[~valid].any()
    # ---- dX, dW, dbias against the products of the materialised gradient
    cos_dx, cos_dw, cos_db = _cos(dx.float(), mat_dx.float()), _cos(dw, mat_dw), _cos(db, mat_db)
    err_dx = ((dx.float() - mat_dx.float()).abs().max() / mat_dx.float().abs().max()).item()
    err_dw = ((dw - mat_dw).abs().max() / mat_dw.abs().max()).item()
    err_db = ((db - mat_db).abs().max() / mat_db.abs().max()).item()
    print(f"dX cos {cos_dx:.6f} max {err_dx:.3e}; dW cos {cos_dw:.6f} max {err_dw:.3e}; dbias cos {cos_db:.6f} max {err_db:.3e}")
    assert min(cos_dx, cos_dw, cos_db) > 0.999, (cos_dx, cos_dw, cos_db)
    assert max(err_dx, err_dw, err_db) < 3e-2, (err_dx, err_dw, err_db)     # (both sides carry dz in bf16: 2^-8 per element)


def test_lm_takes_the_fused_head_at_full_vocabulary(dev):
    """the LM's training step takes the fused head when the gates are met (bf16, V % 8 == 0, d % 64 == 0, enough rows), and its
    loss / gradients agree with the materialised path on the same weights"""
    from types import SimpleNamespace
    from emoasr_amd.modeling.lm import LM
    cfg = dict(lm_type="transformer", vocab_size=10000, hidden_size=256, num_layers=1, num_attention_heads=4,
               intermediate_size=512, max_seq_len=128)
    torch.manual_seed(3)
    lm = LM(SimpleNamespace(**cfg), compute_dtype=torch.bfloat16).to(dev).train()
    lm.hidden_dropout_prob = lm.attention_probs_dropout_prob = 0.0
    B, N = 24, 64
    ys = torch.randint(3, 10000, (B, N))
    ylens = [N - (b % 5) * 7 for b in range(B)]
    labels = torch.randint(3, 10000, (B, N))
    for b, n in enumerate(ylens):
        labels[b, n:] = -100
    out = {}
    for fused in (True, False):
        lm.fused_head = fused
        lm.zero_grad()
        loss, _ = lm(ys, ylens, labels)
        loss.backward()
        assert lm.last_head == ("fused" if fused else "materialised")
        out[fused] = (loss.item(), {n: p.grad.detach().clone() for n, p in lm.named_parameters() if p.grad is not None})
    (lf, gf), (lm_, gm) = out[True], out[False]
    print(f"LM loss: fused {lf:.5f}, materialised {lm_:.5f}")
    assert abs(lf - lm_) < 2e-2 * abs(lm_)
    gmax = max(v.abs().max().item() for v in gm.values())
    for n in gm:
        if gm[n].abs().max() > 1e-2 * gmax:
            assert _cos(gf[n], gm[n]) > 0.98, (n, _cos(gf[n], gm[n]))
