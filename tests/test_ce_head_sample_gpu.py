"""The cross-entropy head that also samples (ops.ce_head_sample_fwd -> emoasr_ce_head_sample_fwd: epilogue mode 7 of the large-tile
product, csrc/gemm_big.hip): soft-max partials, the label's logit and the Gumbel-max sample of every row in one pass, no [M, V] buffer.

  exact     x = 0: the f32 accumulator is 0, so z32 = bias exactly and sample[m] must EQUAL argmax_v f32(bias[v] + g[m, v]) (first
            maximum) with g = ops.gumbel_noise; lse / logp / loss against f64 of the bias row, 1e-6 relative.  Shapes cover one chunk,
            a chunk tail of 8 columns, one full column tile, a tile plus one lane group, a last tile that reaches past ceil(V / 64)
            chunks and the recipe's V; a ragged slab, a ragged row tile and two row tiles at every tile height.
  planted   a dominant value at columns 0, 63, 64, 255, 256, V - 1, one row each, with a random bias: the fold's column arithmetic at
            every boundary.
  product   random bf16 operands: p = z64 + g in f64 (z64 the f64 product of the bf16 operands); per row
            tol = (K + 2) * 2^-23 * max_v (sum_k |x||w| + |bias| + |g|) bounds the f32 accumulation plus the two additions in units of
            2^-23 (so a matrix unit that does not round to nearest is covered).  p[m, sample[m]] >= max p[m] - 2 tol[m] on every row,
            sample[m] == argmax p[m] on every row whose top-two margin exceeds 2 tol; at most 2 % of the rows may fall under that
            margin (a condition on the inputs: 0 rows for these generators).  lse / logp / loss and the gradients through
            ce_head_bwd against ops.ce_head_fwd's on the same inputs, 1e-6 relative to max(1, |.|).
  softmax   4096 identical rows, V = 64: chi-square of the samples against softmax(z64), p > 1e-6."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE


def _bf(t):
    return t.to(torch.bfloat16)


def _inputs(M, V, K, seed, zero_x=False, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(M, K) if zero_x else torch.randn(M, K, generator=g)
    w = torch.randn(V, K, generator=g) * 2 / K ** 0.5
    bias = 0.5 * torch.randn(V, generator=g)
    labels = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    wrow = torch.rand(M, generator=g) + 0.5
    return _bf(x), _bf(w), bias, labels, wrow


def _run(x, w, bias, labels, wrow, seed, row0, dev):
    from emoasr_amd import ops
    assert ops.ce_head_sample_ok(x.to(dev), w.to(dev), 1)
    loss, logp, samples, ctx = ops.ce_head_sample_fwd(x.to(dev), w.to(dev), bias.to(dev), labels.to(dev), wrow.to(dev), seed, row0,
                                                      min_rows=1)
    torch.cuda.synchronize()
    return loss.cpu(), logp.cpu(), samples.cpu().long(), ctx


def _check_exact(dev, M, V, row0):
    from emoasr_amd import ops
    x, w, bias, labels, wrow = _inputs(M, V, 64, 1000 * V + M, zero_x=True)
    loss, logp, samples, ctx = _run(x, w, bias, labels, wrow, SEED, row0, dev)
    noise = ops.gumbel_noise(M, V, SEED, row0, device=dev).cpu()
    want = (bias[None, :] + noise).argmax(dim=1)     # f32 sums on the host; torch's CPU arg-max returns the first maximum
    assert torch.equal(samples, want), (M, V, row0, (samples != want).nonzero().view(-1)[:8].tolist())
    b64 = bias.double()
    lse = torch.logsumexp(b64, 0)
    ref_logp = b64[labels.long()] - lse
    got_lse = ctx[0].cpu().double()
    assert ((got_lse - lse).abs() <= 1e-6 * lse.abs()).all(), (got_lse - lse).abs().max().item()
    assert ((logp.double() - ref_logp).abs() <= 1e-6 * ref_logp.abs()).all(), (logp.double() - ref_logp).abs().max().item()
    ref_loss = -wrow.double() * ref_logp
    assert ((loss.double() - ref_loss).abs() <= 1e-6 * ref_loss.abs()).all(), (loss.double() - ref_loss).abs().max().item()
    assert torch.equal(ctx[1].cpu().long(), labels.long())


@pytest.mark.parametrize("M", [1, 17, 129, 300])
@pytest.mark.parametrize("V", [64, 72, 256, 264, 1000, 10872])
def test_zero_activations_reproduce_the_noise_argmax_exactly(dev, V, M):
    for row0 in (0, 11):
        _check_exact(dev, M, V, row0)


@pytest.mark.parametrize("bm", [128, 192, 256])
def test_every_tile_height(dev, bm):
    from emoasr_amd import lib
    with lib.options(big_bm=bm):
        _check_exact(dev, 300, 1000, 11)


@pytest.mark.parametrize("V", [264, 1000, 10872])
def test_planted_winners_at_the_tile_and_chunk_boundaries(dev, V):
    """row m reads only w[:, m] (x[m] = e_m) and that column is 100 at the planted vocabulary entry, 0 elsewhere: z[m] = bias + 100 at
    one column, exact in bf16 / f32.  The noise spans -2.86 .. 17.4 and the bias a few units, so the planted column must win."""
    cols = [0, 63, 64, 255, 256, V - 1]
    M = len(cols)
    x, w, bias, labels, wrow = _inputs(M, V, 64, V)
    x = torch.zeros_like(x)
    w[:, :M] = 0
    for m, c in enumerate(cols):
        x[m, m] = 1
        w[c, m] = 100
    for row0 in (0, 11):
        _, _, samples, _ = _run(x, w, bias, labels, wrow, SEED, row0, dev)
        assert samples.tolist() == cols, (V, row0, samples.tolist())


_PRODUCT_REF = {}


def _product_case(dev, M, V, K):
    """the inputs, the kernel's outputs and the f64 reference of one product case, computed once"""
    key = (M, V, K)
    if key not in _PRODUCT_REF:
        from emoasr_amd import ops
        x, w, bias, labels, wrow = _inputs(M, V, K, 7 * M + V + K)
        out = _run(x, w, bias, labels, wrow, SEED, 5, dev)
        noise = ops.gumbel_noise(M, V, SEED, 5, device=dev).cpu().double()
        x64, w64 = x.double(), w.double()
        p = x64 @ w64.T + bias.double()[None, :] + noise
        mag = x64.abs() @ w64.abs().T + bias.double().abs()[None, :] + noise.abs()
        tol = (K + 2) * 2.0 ** -23 * mag.max(dim=1).values
        _PRODUCT_REF[key] = (x, w, bias, labels, wrow, out, p, tol)
    return _PRODUCT_REF[key]


PRODUCT_SHAPES = [(300, 1000, 64), (129, 264, 256), (257, 10872, 256)]


@pytest.mark.parametrize("M,V,K", PRODUCT_SHAPES)
def test_samples_with_the_product(dev, M, V, K):
    x, w, bias, labels, wrow, (loss, logp, samples, ctx), p, tol = _product_case(dev, M, V, K)
    top2 = p.topk(2, dim=1).values
    best, margin = top2[:, 0], top2[:, 0] - top2[:, 1]
    chosen = p.gather(1, samples[:, None]).view(-1)
    clear = margin > 2 * tol
    moved = (p.argmax(1) != (x.double() @ w.double().T + bias.double()[None, :]).argmax(1)).float().mean().item()
    print(f"[measured] ce_head_sample M={M} V={V} K={K}: {int((~clear).sum())} of {M} rows inside the margin, worst shortfall "
          f"{((best - chosen) / tol).max().item():.3f} tol, noise moves the arg-max in {100 * moved:.0f} % of rows, "
          f"{int((samples != p.argmax(1)).sum())} samples differ from the f64 arg-max")
    assert ((samples >= 0) & (samples < V)).all()
    assert (~clear).sum().item() <= 0.02 * M, "inputs: too many rows with a top-two margin inside the error bound"
    assert (chosen >= best - 2 * tol).all(), ((best - chosen) / tol).max().item()
    assert torch.equal(samples[clear], p.argmax(1)[clear])


@pytest.mark.parametrize("M,V,K", PRODUCT_SHAPES)
def test_loss_rows_and_gradients_equal_the_logit_free_head(dev, M, V, K, monkeypatch):
    from emoasr_amd import ops
    monkeypatch.setattr(ops, "CE_HEAD_MIN_ROWS", 1)
    x, w, bias, labels, wrow, (loss, logp, samples, ctx), p, tol = _product_case(dev, M, V, K)
    xd, wd, bd, ld, wr = x.to(dev), w.to(dev), bias.to(dev), labels.to(dev), wrow.to(dev)
    assert ops.ce_head_ok(xd, wd)
    loss0, logp0, ctx0 = ops.ce_head_fwd(xd, wd, bd, ld, wr)
    scale = ctx0[0].abs().clamp(min=1.0).cpu()
    bitwise = []
    for name, a, b in (("lse", ctx[0].cpu(), ctx0[0].cpu()), ("logp", logp, logp0.cpu()), ("loss", loss, loss0.cpu())):
        bitwise.append(f"{name} {'bitwise equal' if torch.equal(a, b) else 'max |diff| %.3e' % (a - b).abs().max().item()}")
        assert ((a - b).abs() <= 1e-6 * scale).all(), (name, (a - b).abs().max().item())
    print(f"[measured] ce_head_sample against ce_head M={M} V={V} K={K}: " + ", ".join(bitwise))
    assert torch.equal(ctx[1], ctx0[1])
    grads = []
    for c in (ctx, ctx0):
        dw = torch.zeros(V, K, device=dev)
        db = torch.zeros(V, device=dev)
        dx = ops.ce_head_bwd(xd, wd, bd, c, dw, db, 0.7)
        grads.append((dx.float().cpu(), dw.cpu(), db.cpu()))
    for name, a, b in zip(("dx", "dw", "dbias"), *grads):
        assert ((a - b).abs() <= 1e-6 * b.abs().clamp(min=1.0)).all(), (name, (a - b).abs().max().item())


def test_samples_follow_the_softmax(dev):
    V, R, K = 64, 4096, 64
    g = torch.Generator().manual_seed(V + R)
    xrow = _bf(torch.randn(K, generator=g))
    w = _bf(torch.randn(V, K, generator=g) * 2 / K ** 0.5)
    bias = 0.5 * torch.randn(V, generator=g)
    x = xrow.repeat(R, 1)
    _, _, samples, _ = _run(x, w, bias, torch.zeros(R, dtype=torch.int32), torch.ones(R), 0xE1EC, 0, dev)
    z64 = w.double() @ xrow.double() + bias.double()
    obs = torch.bincount(samples, minlength=V).double()
    assert obs.numel() == V and obs.sum() == R
    exp = torch.softmax(z64, dim=0) * R
    small = exp < 5
    o = torch.cat([obs[~small], obs[small].sum()[None]]) if small.any() else obs
    e = torch.cat([exp[~small], exp[small].sum()[None]]) if small.any() else exp
    stat = ((o - e) ** 2 / e).sum()
    dof = o.numel() - 1
    pv = torch.special.gammaincc(torch.tensor(dof / 2.0, dtype=torch.float64), stat / 2).item()
    print(f"[measured] ce_head_sample samples V={V} R={R}: chi-square {stat.item():.1f} over {dof} degrees of freedom, p = {pv:.3e}")
    assert pv > 1e-6, (stat.item(), dof, pv)
