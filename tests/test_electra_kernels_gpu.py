"""The ELECTRA kernels (csrc/electra.hip) one by one, against float64 references and exact restatements.

  sample_rows      samples EXACTLY argmax(z.float() + gumbel_noise) with ties to the lowest column (the perturbed value is one correctly
                   rounded f32 addition on both sides); loss rows within the bound tests/test_ce_loss_gpu.py derives for lsm_loss at
                   eps = 0: max(4 * e32, (ceil(V / 256) + 10) * 2^-24 * A), e32 the error of the float32 evaluation of the reference
                   on the same case, A = |w * log p[label]|
  distribution     R identical rows are R independent draws from softmax(z): chi-square over the columns (columns with an expected
                   count below 5 pooled into one bin), p-value above 1e-6.  The seed is fixed, so the test is deterministic.  On the
                   CPU, torch.multinomial stays at p >= 9.8e-4 over 200 seeds at (V, R) = (40, 4096) and a 24-bit Gumbel-max
                   restatement at p >= 5.1e-4; at (1000, 16384) they stay at p >= 8.3e-2 and p >= 3.1e-2 over 40 seeds.
  gumbel_noise     a Gumbel(0, 1) variate has mean 0.57722 and variance pi^2 / 6: the block's mean within 4.5 standard errors, its
                   variance within 5 %, every value finite
  electra_corrupt  exact
  bce_head         z, loss and sigmoid within 4 * e32 + (H + 10) * 2^-24 * T, T = sum_c |h[m,c] w_p[c]| + |b_p| the magnitudes of the
                   terms z[m] is the sum of (loss and sigmoid are 1-Lipschitz in z for row weights <= 1, which the cases keep).
                   Backward: dz = w g (sigmoid(z) - y) inherits z's error times w g (sigmoid' <= 1/4), so
                   dh[m,c] within 4 * e32 + w g |w_p[c]| (H + 10) 2^-24 T[m] (+ 2^-8 |ref| of output rounding in bf16),
                   dw_p[c] within 4 * e32 + (M + 10) 2^-24 sum_m |dz h[m,c]| + sum_m |h[m,c]| w g (H + 10) 2^-24 T[m], db_p likewise
                   with h = 1.  The sums into dw_p / db_p are f32 atomics: only their order is free."""
import math

import numpy as np
import pytest
import torch

from tests.ctc_ref import lsm_ref
from tests.test_ce_loss_gpu import _f32, _i32, _strided

pytestmark = pytest.mark.gpu

P24, P8 = 2.0 ** -24, 2.0 ** -8
_DT = [torch.float32, torch.bfloat16]
_DT_IDS = ["f32", "bf16"]
EULER = 0.5772156649015329


def _want_samples(z, noise):
    """first maximum of the f32 sums, on the host"""
    return np.argmax((z.float() + noise.cpu()).numpy(), axis=1)


# ---- sample_rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [2, 3, 255, 256, 257, 1000, 9798])
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_sample_rows(dev, dtype, V):
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(V)
    M, seed, row0 = 5, 0x5EED0001, 3
    z = (torch.randn(M, V, generator=g) * 2).to(dtype)
    labels = [0, V - 1, int(torch.randint(0, V, (1,), generator=g)), V - 1, 0]
    w = [0.5, 1.0, 0.0, 0.25, 2.0]
    zd = _strided(z, dev)
    assert zd.stride(0) == V + 5
    lab_d, w_d = _i32(labels, dev), _f32(w, dev)
    loss, samples, lse = ops.sample_rows(zd, lab_d, w_d, seed, row0=row0, want_lse=True)
    noise = ops.gumbel_noise(M, V, seed, row0=row0, device=dev)
    assert torch.isfinite(noise).all()
    got = samples.cpu().numpy()
    assert got.dtype == np.int32 and ((got >= 0) & (got < V)).all()
    assert np.array_equal(got, _want_samples(z, noise)), (got, _want_samples(z, noise))
    # loss rows, log-sum-exp
    z64 = z.double().numpy()
    ref, m32 = lsm_ref(z64, labels, w, 0.0), lsm_ref(z64, labels, w, 0.0, dtype=np.float32)
    e32 = float(np.abs(m32.loss.astype(np.float64) - ref.loss).max())
    bound = np.maximum(4 * e32, (math.ceil(V / 256) + 10) * P24 * ref.mag)
    err = np.abs(loss.cpu().numpy().astype(np.float64) - ref.loss)
    print(f"[measured] sample_rows V={V} {dtype}: loss err {err.max():.2e} (f32 model {e32:.2e}), {float((err / (bound + 1e-300)).max()):.2f} of bound")
    assert (err <= bound).all(), (err, bound)
    assert loss[2].item() == 0.0
    lse64 = torch.logsumexp(z.double(), dim=1).numpy()
    assert np.abs(lse.cpu().numpy() - lse64).max() <= (math.ceil(V / 256) + 10) * P24 * np.abs(lse64).max() + 4 * P24
    # the same seed: the same bits; without the lse output too
    loss2, samples2, none = ops.sample_rows(zd, lab_d, w_d, seed, row0=row0)
    assert none is None and torch.equal(loss2, loss) and torch.equal(samples2, samples)
    # chunks of rows draw what one call draws
    la, sa, _ = ops.sample_rows(zd[:2], lab_d[:2], w_d[:2], seed, row0=row0)
    lb, sb, _ = ops.sample_rows(zd[2:], lab_d[2:], w_d[2:], seed, row0=row0 + 2)
    assert torch.equal(torch.cat([sa, sb]), samples) and torch.equal(torch.cat([la, lb]), loss)
    if V >= 1000:     # another seed, other samples (five draws from a flat-tailed distribution over >= 1000 columns)
        _, other, _ = ops.sample_rows(zd, lab_d, w_d, seed + 1, row0=row0)
        assert not torch.equal(other, samples)
        _, moved, _ = ops.sample_rows(zd, lab_d, w_d, seed, row0=row0 + 1)
        assert not torch.equal(moved, samples)


@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_sample_rows_takes_a_dominant_column_and_breaks_ties_low(dev, dtype):
    """a logit 40 above the rest is sampled whatever the noise (its range is 20.3 wide); equal perturbed values go to the lowest column"""
    from emoasr_amd import ops
    V = 777
    z = torch.zeros(4, V)
    for m, c in enumerate((0, 300, 776, 255)):
        z[m, c] = 40.0
    zd = _strided(z.to(dtype), dev)
    _, samples, _ = ops.sample_rows(zd, _i32([0] * 4, dev), _f32([1.0] * 4, dev), 99)
    assert samples.cpu().tolist() == [0, 300, 776, 255]
    # ties: every logit so large that adding the noise (|g| < 32) rounds back to the logit itself
    big = torch.full((3, 600), 2.0 ** 31).to(dtype)
    _, samples, _ = ops.sample_rows(big.to(dev), _i32([0] * 3, dev), _f32([1.0] * 3, dev), 5)
    assert samples.cpu().tolist() == [0, 0, 0]
    big[1, :257] = 0.0
    big[2, :599] = 0.0
    _, samples, _ = ops.sample_rows(big.to(dev), _i32([0] * 3, dev), _f32([1.0] * 3, dev), 5)
    assert samples.cpu().tolist() == [0, 257, 599]


@pytest.mark.parametrize("V,R", [(40, 4096), (1000, 16384)])
def test_samples_follow_the_softmax(dev, V, R):
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(V + R)
    z = (torch.randn(V, generator=g) * 2.5).to(torch.bfloat16)
    zd = z.to(dev).repeat(R, 1)
    _, samples, _ = ops.sample_rows(zd, torch.zeros(R, dtype=torch.int32, device=dev), torch.ones(R, device=dev), 0xE1EC)
    obs = torch.bincount(samples.cpu().long(), minlength=V).double()
    assert obs.numel() == V and obs.sum() == R
    exp = torch.softmax(z.double(), dim=0) * R
    small = exp < 5
    o = torch.cat([obs[~small], obs[small].sum()[None]]) if small.any() else obs
    e = torch.cat([exp[~small], exp[small].sum()[None]]) if small.any() else exp
    stat = ((o - e) ** 2 / e).sum()
    dof = o.numel() - 1
    p = torch.special.gammaincc(torch.tensor(dof / 2.0, dtype=torch.float64), stat / 2).item()
    print(f"[measured] samples V={V} R={R}: chi-square {stat.item():.1f} over {dof} degrees of freedom, p = {p:.3e}")
    assert p > 1e-6, (stat.item(), dof, p)


def test_gumbel_noise_statistics(dev):
    from emoasr_amd import ops
    x = ops.gumbel_noise(64, 4096, 0xABCDEF, row0=11, device=dev).double().cpu()
    n = x.numel()
    assert torch.isfinite(x).all()
    var = math.pi ** 2 / 6
    mean_err = abs(x.mean().item() - EULER) / math.sqrt(var / n)
    print(f"[measured] gumbel_noise: mean {x.mean().item():.5f} ({mean_err:.2f} standard errors), variance {x.var().item():.5f} "
          f"against {var:.5f}, range {x.min().item():.3f} .. {x.max().item():.3f}")
    assert mean_err <= 4.5 and abs(x.var().item() - var) <= 0.05 * var
    assert not torch.equal(x, ops.gumbel_noise(64, 4096, 0xABCDEF + 1, row0=11, device=dev).double().cpu())
    # row0 shifts the block: rows 1.. of one call are rows 0.. of the next
    y = ops.gumbel_noise(63, 4096, 0xABCDEF, row0=12, device=dev).double().cpu()
    assert torch.equal(x[1:], y)


# ---- electra_corrupt -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 7, 9])
@pytest.mark.parametrize("case", ["none", "all", "some"])
def test_electra_corrupt_exact(dev, N, case):
    from emoasr_amd import ops
    B, mask_id, pad = 3, 39, 8
    g = torch.Generator().manual_seed(10 * N + len(case))
    ids = torch.randint(3, 39, (B, N), generator=g, dtype=torch.int32)
    if case == "none":
        rows = []
    elif case == "all":
        rows = list(range(B * N))
    else:
        rows = sorted(torch.randperm(B * N, generator=g)[: max(2, B * N // 3)].tolist())
    M = len(rows)
    labels = torch.randint(3, 39, (M,), generator=g, dtype=torch.int32)
    samples = torch.randint(0, 40, (M,), generator=g, dtype=torch.int32)
    if M >= 1:
        samples[0] = labels[0]          # the generator drew the hidden token: not replaced
    if M >= 2:
        samples[1] = mask_id            # the mask token itself is a sample like any other: replaced
        labels[1] = 5
    masked = ids.clone().view(-1)
    for r in rows:
        masked[r] = mask_id
    # restatement: electra.py:80-86
    generated, original = masked.clone(), masked.clone()
    for m, r in enumerate(rows):
        generated[r], original[r] = samples[m], labels[m]
    replaced = (generated != original).float()
    gen_buf = torch.full((B * N + pad,), -7, dtype=torch.int32, device=dev)
    rep_buf = torch.full((B * N + pad,), float("nan"), device=dev)
    cnt_buf = torch.full((2 + pad,), -7, dtype=torch.int32, device=dev)
    ops.electra_corrupt(masked.view(B, N).to(dev), _i32(rows, dev), labels.to(dev), samples.to(dev), out=(gen_buf, rep_buf, cnt_buf))
    torch.cuda.synchronize()
    assert torch.equal(gen_buf[: B * N].cpu(), generated) and torch.equal(rep_buf[: B * N].cpu(), replaced)
    assert cnt_buf[:2].cpu().tolist() == [int(replaced.sum()), M]
    assert (gen_buf[B * N:] == -7).all() and torch.isnan(rep_buf[B * N:]).all() and (cnt_buf[2:] == -7).all()
    if M >= 2:
        assert replaced[rows[0]] == 0 and replaced[rows[1]] == 1 and generated[rows[1]] == mask_id
    # fresh buffers, shaped like the ids
    gen2, rep2, cnt2 = ops.electra_corrupt(masked.view(B, N).to(dev), _i32(rows, dev), labels.to(dev), samples.to(dev))
    assert gen2.shape == (B, N) and torch.equal(gen2.cpu().view(-1), generated) and torch.equal(rep2.cpu().view(-1), replaced)
    assert cnt2.cpu().tolist() == [int(replaced.sum()), M]


# ---- bce_head ------------------------------------------------------------------------------------------------------------------------
def _bce_ref(h, wp, b, y, w, g, dtype):
    h, wp, y, w = (np.asarray(a).astype(dtype) for a in (h, wp, y, w))
    b, g = dtype(b), dtype(g)
    z = h @ wp + b
    loss = w * (np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z))))
    sig = 1 / (1 + np.exp(-z))
    dz = w * (sig - y) * g
    return dict(z=z, loss=loss, sig=sig, dz=dz, dh=dz[:, None] * wp[None, :], dw=dz @ h, db=dz.sum(keepdims=True))


@pytest.mark.parametrize("M", [1, 5, 300])
@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_bce_head(dev, dtype, H, M):
    from emoasr_amd import ops
    gen = torch.Generator().manual_seed(H + M)
    wp = (torch.randn(H, generator=gen) * 0.3).to(dtype)
    h = torch.randn(M, H, generator=gen)
    unit = wp.float() / (wp.float() ** 2).sum()
    h[0] = 60.0 * unit                      # z = +60: sigmoid saturated at 1
    if M > 1:
        h[1] = -60.0 * unit                 # z = -60: at 0
    h = h.to(dtype)
    b = 0.125
    y = (torch.rand(M, generator=gen) < 0.4).float()
    w = torch.rand(M, generator=gen)        # <= 1
    if M > 2:
        w[2] = 0.0
    gs, gdev = 2.0, 0.25
    h64, wp64 = h.double().numpy(), wp.double().numpy()
    ref = _bce_ref(h64, wp64, b, y.numpy(), w.numpy(), gs * gdev, np.float64)
    m32 = _bce_ref(h64, wp64, b, y.numpy(), w.numpy(), gs * gdev, np.float32)
    e32 = {k: float(np.abs(m32[k].astype(np.float64) - ref[k]).max()) for k in ref}
    assert np.abs(ref["z"]).max() > 59
    T = (np.abs(h64) * np.abs(wp64)[None, :]).sum(axis=1) + abs(b)
    bz = (H + 10) * P24 * T
    hd, wd, bd, yd, wgt = h.to(dev), wp.to(dev), _f32([b], dev), y.to(dev), w.to(dev)
    z, loss, sig = ops.bce_head_fwd(hd, wd, bd, yd, wgt, want_sigmoid=True)
    lines = []
    for name, got in (("z", z), ("loss", loss), ("sig", sig)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref[name])
        bound = 4 * e32[name] + bz
        lines.append(f"{name} {err.max():.2e} ({float((err / bound).max()):.2f} of bound)")
        assert np.isfinite(got.cpu().numpy()).all() and (err <= bound).all(), (name, err.max(), bound.min())
    if M > 2:
        assert loss[2].item() == 0.0
    z2, none, sig2 = ops.bce_head_fwd(hd, wd.view(1, H), bd, want_sigmoid=True)     # the score path: no targets
    assert none is None and torch.equal(z2, z) and torch.equal(sig2, sig)
    # backward, twice into the same slots
    dw, db = torch.zeros(H, device=dev), torch.zeros(1, device=dev)
    wg = w.numpy().astype(np.float64) * gs * gdev
    dz_err = wg * bz
    b_dh = 4 * e32["dh"] + dz_err[:, None] * np.abs(wp64)[None, :] + (P8 * np.abs(ref["dh"]) if dtype == torch.bfloat16 else 0.0)
    b_dw = 4 * e32["dw"] + (M + 10) * P24 * (np.abs(ref["dz"])[:, None] * np.abs(h64)).sum(axis=0) + (np.abs(h64) * dz_err[:, None]).sum(axis=0)
    b_db = 4 * e32["db"] + (M + 10) * P24 * np.abs(ref["dz"]).sum() + dz_err.sum()
    for k in (1, 2):
        dh = ops.bce_head_bwd(hd, wd, z, yd, wgt, dw, db, gs, torch.tensor([gdev], device=dev))
        e_dh = np.abs(dh.float().cpu().numpy().astype(np.float64) - ref["dh"])
        e_dw = np.abs(dw.cpu().numpy().astype(np.float64) - k * ref["dw"])
        e_db = np.abs(db.cpu().numpy().astype(np.float64) - k * ref["db"])
        assert dh.dtype == dtype and (e_dh <= b_dh).all(), (k, e_dh.max())
        assert (e_dw <= k * b_dw).all() and (e_db <= k * b_db).all(), (k, e_dw.max(), e_db.max())
    lines.append(f"dh {e_dh.max():.2e} ({float((e_dh / (b_dh + 1e-300)).max()):.2f}) dw {float((e_dw / (2 * b_dw)).max()):.2f} db {float((e_db / (2 * b_db)).max()):.2f}")
    print(f"[measured] bce_head H={H} M={M} {dtype}: " + ", ".join(lines))
    if M > 2:
        assert not dh[2].any()
