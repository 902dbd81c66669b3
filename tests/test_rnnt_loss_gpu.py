"""The transducer's loss side at kernel level: csrc/rnnt.hip (row gather, lattice, gradient rows, joint broadcast / reductions, row
arg-max, first-not-equal) and the two transducer epilogues of the large-tile product (csrc/gemm_big.hip) against the float64
reference of tests/rnnt_ref.py (pinned on the CPU by tests/test_rnnt_ref_cpu.py), at the lattice and vocabulary edges where the
kernels change path: anti-diagonal counts around the 8-diagonal prefetch chunk, one / two / three waves of label positions, the full
1024-thread block, the 16-byte register rows and the scalar fall-back of both dtypes, partial 64-column chunks, every tile height.

Bounds (none taken from the kernels under test):
  f32 lattice quantities   |got - ref64| <= max(4 * e32, floor): e32 = the error of the float32 evaluation of the same formulas
                           (rnnt_ref(dtype=float32), libm accuracy) on the same case; floor = the suite's existing 1e-4 (absolute or
                           relative) for nll / alpha / beta / lse / lpb / lpy and 1e-5 * gs / 0.25 for the gradient.  The factor 4: the
                           hardware exp2 / log2 units (a few ulp against libm's half) and another summation order.
  bf16 gradient            the f32 bound + 2^-8 |ref| (one bf16 ulp of output rounding)
  fused head               2e-3 (nll, lse, lpb, lpy), 3e-3 of the largest gradient entry (gradient rows, row constants)
  joint_tanh / joint_reduce  stated at the tests
  indices, "bit-identical"   exact"""
import functools

import numpy as np
import pytest
import torch

from tests.rnnt_ref import rnnt_ref

pytestmark = pytest.mark.gpu

P23, P8 = 2.0 ** -23, 2.0 ** -8


def _i32(a, dev):
    return torch.as_tensor(np.asarray(a)).to(torch.int32).to(dev)


def _labels(g, B, L, V, blank):
    lab = torch.randint(0, V - 1, (B, L), generator=g)
    return lab + (lab >= blank).long()     # any symbol but the blank


def _worst(got, ref, bound):
    """max of |got - ref| / bound over the entries where ref is finite; the others must be equal (+-inf in place)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]), "infinite entries differ"
    if not fin.any():
        return 0.0, 0.0
    assert np.isfinite(got[fin]).all(), "non-finite value where the reference is finite"
    err = np.abs(got[fin] - ref[fin])
    return float(err.max()), float((err / np.broadcast_to(bound, ref.shape)[fin]).max())     # (arrays of one shape, or a scalar bound)


def _e32(m32, ref, sel=None):
    a, b = np.asarray(m32, np.float64), np.asarray(ref, np.float64)
    if sel is not None:
        a, b = a[sel], b[sel]
    fin = np.isfinite(b)
    return float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0


def _check_materialised(dev, name, z, labels, elens, ylens, blank, gs, gscale_dev=None):
    """ops.rnnt_forward + ops.rnnt_grad on z (CPU tensor, f32 or bf16) against the float64 reference on the same rounded logits.
    -> (ctx, nll, dz) device tensors and the reference"""
    from emoasr_amd import ops
    z64 = z.double().numpy()
    gs_total = gs * (1.0 if gscale_dev is None else float(gscale_dev))
    ref = rnnt_ref(z64, labels, elens, ylens, blank, gs=gs_total)
    m32 = rnnt_ref(z64, labels, elens, ylens, blank, gs=gs_total, dtype=np.float32)
    zd = z.to(dev)
    L, E, Y = _i32(labels, dev), _i32(elens, dev), _i32(ylens, dev)
    ctx, nll = ops.rnnt_forward(zd, L, E, Y, blank)
    # NaN-filled, with a guard behind the last row: an unwritten row and a store past the tensor's end both show
    flat = torch.full((zd.numel() + 64,), float("nan"), device=dev, dtype=zd.dtype)
    out = flat[:zd.numel()].view_as(zd)
    gdev = None if gscale_dev is None else torch.tensor([gscale_dev], device=dev, dtype=torch.float32)
    dz = ops.rnnt_grad(zd, ctx, nll, L, E, Y, blank, gs, gscale_dev=gdev, out=out)
    assert dz.data_ptr() == out.data_ptr()
    assert bool(torch.isnan(flat[zd.numel():]).all()), f"{name}: the gradient kernel stored past the end of its rows"
    got = dict(zip(("lse", "lpb", "lpy", "alpha", "beta"), (c.cpu().numpy() for c in ctx)))
    got["nll"] = nll.cpu().numpy()
    lines = []
    for k in ("lse", "lpb", "lpy", "alpha", "beta", "nll"):
        sel = ref.valid if k in ("alpha", "beta") else None     # (the kernel leaves alpha / beta outside the lattice unwritten)
        r = getattr(ref, k) if sel is None else getattr(ref, k)[sel]
        g = got[k] if sel is None else got[k][sel]
        e32 = _e32(getattr(m32, k), getattr(ref, k), sel)
        bound = np.maximum(4 * e32, 1e-4 * np.maximum(1.0, np.abs(np.where(np.isfinite(r), r, 0.0))))
        err, ratio = _worst(g, r, bound)
        lines.append((k, err, e32, ratio))
    dzc = dz.float().cpu().numpy()
    assert np.isfinite(dzc).all(), f"{name}: gradient rows left unwritten (NaN fill) or non-finite"
    e32 = _e32(m32.dz, ref.dz)
    bound = np.maximum(4 * e32, 1e-5 * gs_total / 0.25)
    if z.dtype == torch.bfloat16:
        bound = bound + P8 * np.abs(ref.dz)
    err, ratio = _worst(dzc, ref.dz, bound)
    lines.append(("dz", err, e32, ratio))
    print(f"[measured] rnnt {name}: " + ", ".join(f"{k} err {e:.2e} (f32 model {m:.2e}) {r:.2f} of bound" for k, e, m, r in lines))
    for k, e, m, r in lines:
        assert r <= 1.0, (name, k, e, m, r)
    assert (dzc[~ref.valid] == 0).all(), f"{name}: non-zero gradient outside the lattice"
    return ctx, nll, dz, ref


# ---- lattice geometry: f32, V = 8 (the f32 register row) ----------------------------------------------------------------------
@pytest.mark.parametrize("blank", [0, 3, 7])
def test_lattice_diagonal_counts_around_the_prefetch_chunk(dev, blank):
    """T + Ub in {1, 8, 9, 16, 17} (the 8-diagonal chunk: exactly one, one + 1, two, two + 1), one frame with three labels, a row of
    one repeated symbol and an utterance without frames (nll = +inf, zero rows) -- ragged, in ONE launch"""
    g = torch.Generator().manual_seed(10 + blank)
    T, U, V = 10, 8, 8
    elens = [1, 5, 5, 10, 10, 1, 0, 10]
    ylens = [0, 3, 4, 6, 7, 3, 2, 7]
    B = len(elens)
    z = torch.randn(B, T, U, V, generator=g) * 2
    labels = _labels(g, B, U - 1, V, blank)
    labels[7] = (blank + 2) % V
    ctx, nll, dz, ref = _check_materialised(dev, f"diagonals blank={blank}", z, labels, elens, ylens, blank, 1.0 / B)
    assert torch.isposinf(nll[6]) and bool((dz[6] == 0).all())
    assert sorted({min(e, T) + y for e, y in zip(elens, ylens) if e}) == [1, 4, 8, 9, 16, 17]


def test_lattice_without_labels(dev):
    g = torch.Generator().manual_seed(20)
    B, T, U, V = 3, 7, 3, 8
    z = torch.randn(B, T, U, V, generator=g) * 2
    _check_materialised(dev, "no labels", z, _labels(g, B, U - 1, V, 0), [7, 1, 4], [0, 0, 0], 0, 1.0)


@pytest.mark.parametrize("U", [64, 65, 128, 129])
def test_lattice_exchange_between_waves(dev, U):
    """label positions that fill one wave exactly, spill one into the second, fill two, spill into the third; in the same block
    shorter label rows that end on and around the wave boundary (Ub = 63, 64, 65 where they fit)"""
    g = torch.Generator().manual_seed(U)
    B, T, V = 4, 6, 8
    ylens = [U - 1, min(U - 1, 63), min(U - 1, 64), min(U - 1, 65)]
    z = torch.randn(B, T, U, V, generator=g) * 2
    _check_materialised(dev, f"waves U={U}", z, _labels(g, B, U - 1, V, 0), [6, 5, 3, 6], ylens, 0, 1.0 / B)


def test_lattice_full_block_and_the_limit(dev):
    """U = 1024: every thread of the largest block owns a label position.  U = 1025 is refused before anything is launched."""
    from emoasr_amd import lib, ops
    g = torch.Generator().manual_seed(30)
    B, T, U, V = 2, 2, 1024, 8
    z = torch.randn(B, T, U, V, generator=g) * 2
    _check_materialised(dev, "U=1024", z, _labels(g, B, U - 1, V, 0), [2, 1], [1023, 500], 0, 0.5)
    U = 1025
    z = torch.randn(1, 1, U, V, generator=g).to(dev)
    lab, one = torch.ones(1, U - 1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    with pytest.raises(lib.EmoasrHipError, match="exceeds 1024"):
        ops.rnnt_forward(z, lab, one, one, 0)
    bufs = [torch.full((1, 1, U), 7.0, device=dev) for _ in range(5)] + [torch.full((1,), 7.0, device=dev)]
    with pytest.raises(lib.EmoasrHipError, match="exceeds 1024"):
        lib.call("emoasr_rnnt_forward", ops.dt(z), 1, 1, U, V, U - 1, ops._p(z), ops._p(lab), ops._p(one), ops._p(one), 0,
                 *[ops._p(b) for b in bufs], ops._stream())
    torch.cuda.synchronize()
    assert all(bool((b == 7.0).all()) for b in bufs)     # not even the row gather ran


def test_long_lattice_and_lengths_past_the_tensor(dev):
    """T = 120, Ub = 40 (160 diagonals: twenty chunks) next to T = 90, Ub = 17; elens = T + 5 is clamped to the tensor: the same bits"""
    g = torch.Generator().manual_seed(40)
    B, T, U, V = 2, 120, 41, 8
    z = torch.randn(B, T, U, V, generator=g) * 2
    labels = _labels(g, B, U - 1, V, 0)
    ctx, nll, dz, ref = _check_materialised(dev, "long", z, labels, [120, 90], [40, 17], 0, 1.0)
    ctx5, nll5, dz5, _ = _check_materialised(dev, "long, elens + 5", z, labels, [125, 90], [40, 17], 0, 1.0)
    assert torch.equal(nll, nll5) and torch.equal(dz, dz5)
    valid = torch.from_numpy(ref.valid).to(dev)
    for a, b in zip(ctx, ctx5):
        assert torch.equal(a[valid], b[valid])


# ---- vocabulary paths -----------------------------------------------------------------------------------------------------------
# f32: registers + 16-byte loads for V % 4 == 0 && V <= 1024 (gather) / V % 4 == 0 (gradient); bf16: V % 8 == 0 && V <= 2048 / V % 8 == 0
_VOCABS = [(torch.float32, v) for v in (4, 17, 252, 1000, 1024, 1028, 1030)] + \
          [(torch.bfloat16, v) for v in (8, 17, 1000, 2048, 2056, 2050)]


def _vocab_case(dtype, V, last_blank, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + V)
    B, T, U = 2, 5, 4
    blank = V - 1 if last_blank else 0
    z = (torch.randn(B, T, U, V, generator=g) * 2).to(dtype)
    labels = _labels(g, B, U - 1, V, blank)
    labels[:, 0] = V - 2 if last_blank else V - 1     # a label in the row's last (partial) vector, next to the blank / far from it
    return z, labels, [5, 3], [3, 1], blank


@pytest.mark.parametrize("last_blank", [True, False], ids=["blank_last", "blank_first"])
@pytest.mark.parametrize("dtype,V", _VOCABS, ids=[f"{'f32' if d == torch.float32 else 'bf16'}-{v}" for d, v in _VOCABS])
def test_vocabulary_paths(dev, dtype, V, last_blank):
    z, labels, elens, ylens, blank = _vocab_case(dtype, V, last_blank)
    _check_materialised(dev, f"V={V} {str(dtype)[6:]} blank={blank}", z, labels, elens, ylens, blank, 0.5)


def test_softmax_stability_with_spiked_rows(dev):
    """every row: one +60 among values near -60 (exp(z - max) underflows everywhere else; without the max it overflows)"""
    g = torch.Generator().manual_seed(50)
    B, T, U, V, blank = 2, 5, 4, 1000, 0
    z = torch.randn(B, T, U, V, generator=g) - 60
    labels = _labels(g, B, U - 1, V, blank)
    labels[:, 0] = V - 1
    for b in range(B):
        for t in range(T):
            for u in range(U):
                cands = [blank, int(labels[b, min(u, U - 2)]), int(torch.randint(0, V, (1,), generator=g))]
                z[b, t, u, cands[int(torch.randint(0, 3, (1,), generator=g))]] = 60.0
    _check_materialised(dev, "spiked rows", z, labels, [5, 3], [3, 1], blank, 0.5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gradient_scale_from_a_device_scalar(dev, dtype):
    """gscale_dev (the loss scale lives on the device): gscale * gscale_dev[0], the bits of the same product passed as gscale"""
    z, labels, elens, ylens, blank = _vocab_case(dtype, 1000, True, seed=1)
    _, _, dz_dev, _ = _check_materialised(dev, f"gscale_dev {str(dtype)[6:]}", z, labels, elens, ylens, blank, 0.5, gscale_dev=0.25)
    _, _, dz_host, _ = _check_materialised(dev, f"gscale 0.125 {str(dtype)[6:]}", z, labels, elens, ylens, blank, 0.125)
    assert torch.equal(dz_dev, dz_host)


# ---- fused head: the output layer + lattice without the logits ----------------------------------------------------------------------
_HEAD_SHAPES = [(64, 64), (72, 64), (256, 512), (264, 64), (1000, 512)]


@functools.lru_cache(maxsize=None)
def _head_case(V, J, many_rows, last_blank):
    """inputs (CPU) + the float64 reference on z = h W^T + b of the bf16 h, W and the f32 bias; built once, shared by every tile height"""
    g = torch.Generator().manual_seed(V * 7 + J + 2 * many_rows + last_blank)
    if many_rows:
        B, T, U = 4, 37, 10                         # 1480 cells: six 256-row tiles, the last one ragged
        elens, ylens = [37, 30, 11, 2], [9, 5, 0, 7]
    else:
        B, T, U = 2, 3, 4                           # 24 cells: less than one tile
        elens, ylens = [3, 2], [3, 3]
    blank = V - 1 if last_blank else 0
    h = torch.tanh(torch.randn(B * T * U, J, generator=g)).to(torch.bfloat16)
    w = (torch.randn(V, J, generator=g) / J ** 0.5 * 3).to(torch.bfloat16)
    bias = torch.randn(V, generator=g) * 0.5
    bias[blank] += 2.0
    labels = _labels(g, B, U - 1, V, blank)
    # labels on the last column, next to it, and on both sides of the 64- and 256-column boundaries (where the vocabulary has them)
    forced = [c for c in (V - 1, 63, 64, 255, 256, V - 2) if c < V]
    forced = list(dict.fromkeys(forced))
    flat = labels.view(-1)
    slots = [b * (U - 1) + u for u in range(U - 1) for b in range(B) if u < ylens[b]]     # u-major: spread over the utterances
    if many_rows:
        slots = list(range(U - 1))                                                     # utterance 0 holds nine labels
    for s, c in zip(slots, forced):
        flat[s] = c
    used = {int(labels[b, u]) for b in range(B) for u in range(ylens[b])}
    assert set(forced) <= used, (forced, used)
    z64 = (h.double() @ w.double().t() + bias.double()).view(B, T, U, V).numpy()
    gs = 1.0 / B
    ref = rnnt_ref(z64, labels, elens, ylens, blank, gs=gs)
    return dict(B=B, T=T, U=U, V=V, J=J, blank=blank, h=h, w=w, bias=bias, labels=labels, elens=elens, ylens=ylens, gs=gs, ref=ref)


def _close_2e3(got, ref):
    r = np.where(np.isfinite(ref), ref, 0.0)
    return _worst(got, ref, 2e-3 + 2e-3 * np.abs(r))


@pytest.mark.parametrize("bm", [0, 256, 192, 128])
@pytest.mark.parametrize("many_rows", [False, True], ids=["24rows", "1480rows"])
@pytest.mark.parametrize("V,J", _HEAD_SHAPES)
def test_fused_head(dev, V, J, many_rows, bm):
    """ops.rnnt_head_forward / rnnt_coef / rnnt_head_grad at every tile height: one chunk (V = 64), a last chunk of 8 columns
    (V = 72, 264), full column tiles (256) and the L4 width (1000: a last chunk of 40); blank first and last; labels on the last
    column and on both sides of the 64- / 256-column boundaries; fewer rows than a tile and a ragged last tile"""
    from emoasr_amd import lib, ops
    for last_blank in (False, True):
        c = _head_case(V, J, many_rows, last_blank)
        B, T, U, blank, ref, gs = c["B"], c["T"], c["U"], c["blank"], c["ref"], c["gs"]
        N = B * T * U
        hd, wd, bd = c["h"].to(dev), c["w"].to(dev), c["bias"].to(dev)
        L, E, Y = _i32(c["labels"], dev), _i32(c["elens"], dev), _i32(c["ylens"], dev)
        with lib.options(big_bm=bm):
            ctx, nll = ops.rnnt_head_forward(hd, wd, bd, B, T, U, L, E, Y, blank)
            coef, ycol = ops.rnnt_coef(ctx, nll, L, E, Y, gs)
            dz = torch.full((N, V), float("nan"), device=dev, dtype=torch.bfloat16)
            r0 = 0
            for n in (7, 500, 300, N):     # uneven chunks
                n = min(n, N - r0)
                if n:
                    ops.rnnt_head_grad(hd[r0:r0 + n], wd, bd, coef[r0:r0 + n], ycol[r0:r0 + n], blank, dz[r0:r0 + n])
                r0 += n
        res = {}
        for k, t in zip(("lse", "lpb", "lpy"), ctx):
            res[k] = _close_2e3(t.cpu().numpy(), getattr(ref, k))
        res["nll"] = _close_2e3(nll.cpu().numpy(), ref.nll)
        # index-valued: exact
        want_ycol = np.full((B, T, U), -1, np.int64)
        for b in range(B):
            Tb, Ub = min(c["elens"][b], T), c["ylens"][b]
            want_ycol[b, :Tb, :Ub] = c["labels"][b, :Ub].numpy()[None, :]
        assert np.array_equal(ycol.cpu().numpy().reshape(B, T, U), want_ycol)
        gmax = float(np.abs(ref.dz).max())
        cf = coef.cpu().numpy().reshape(B, T, U, 4)
        res["coef lse"] = _close_2e3(cf[..., 0], ref.lse)
        for i, (k, want) in enumerate((("occ", ref.gb + ref.gy), ("gb", ref.gb), ("gy", ref.gy)), 1):
            res["coef " + k] = _worst(cf[..., i], want * gs, 3e-3 * gmax)
            assert (cf[..., i][~ref.valid] == 0).all()
        dzc = dz.float().cpu().numpy().reshape(B, T, U, V)
        assert np.isfinite(dzc).all(), "gradient rows left unwritten (NaN fill) or non-finite"
        res["dz"] = _worst(dzc, ref.dz, 3e-3 * gmax)
        assert (dzc[~ref.valid] == 0).all()
        print(f"[measured] fused head V={V} J={J} rows={N} blank={blank} bm={bm}: "
              + ", ".join(f"{k} err {e:.2e} {r:.2f} of bound" for k, (e, r) in res.items()))
        for k, (e, r) in res.items():
            assert r <= 1.0, (k, e, r)


@pytest.mark.parametrize("bm", [0, 256, 192, 128])
@pytest.mark.parametrize("V,J", [(264, 64), (1000, 512)])
def test_fused_head_in_several_launches(dev, V, J, bm):
    """rows_per_launch = 256 on 1480 cells: six launches, five of them with row0 > 0 (reached in production only above 4 GiB of
    joint activations) -- the bits of the single launch"""
    from emoasr_amd import lib, ops
    c = _head_case(V, J, True, False)
    B, T, U, blank = c["B"], c["T"], c["U"], c["blank"]
    hd, wd, bd = c["h"].to(dev), c["w"].to(dev), c["bias"].to(dev)
    L, E, Y = _i32(c["labels"], dev), _i32(c["elens"], dev), _i32(c["ylens"], dev)
    with lib.options(big_bm=bm):
        ctx1, nll1 = ops.rnnt_head_forward(hd, wd, bd, B, T, U, L, E, Y, blank)
        ctx6, nll6 = ops.rnnt_head_forward(hd, wd, bd, B, T, U, L, E, Y, blank, rows_per_launch=256)
    valid = torch.from_numpy(c["ref"].valid).to(dev)
    assert torch.equal(nll1, nll6)
    for k, a, b in zip(("lse", "lpb", "lpy", "alpha", "beta"), ctx1, ctx6):
        if k in ("alpha", "beta"):
            a, b = a[valid], b[valid]
        assert torch.equal(a, b), k
    assert _close_2e3(nll6.cpu().numpy(), c["ref"].nll)[1] <= 1.0
    with pytest.raises(AssertionError):
        ops.rnnt_head_forward(hd, wd, bd, B, T, U, L, E, Y, blank, rows_per_launch=100)


def test_fused_head_lattice_on_a_side_stream(dev):
    """lattice_stream: the fold + lattice on a side stream; after the returned event, the bits of the same-stream call"""
    from emoasr_amd import ops
    c = _head_case(1000, 512, True, False)
    B, T, U, blank = c["B"], c["T"], c["U"], c["blank"]
    hd, wd, bd = c["h"].to(dev), c["w"].to(dev), c["bias"].to(dev)
    L, E, Y = _i32(c["labels"], dev), _i32(c["elens"], dev), _i32(c["ylens"], dev)
    ctx1, nll1 = ops.rnnt_head_forward(hd, wd, bd, B, T, U, L, E, Y, blank)
    side = torch.cuda.Stream(device=dev)
    ctx2, nll2, ev, keep = ops.rnnt_head_forward(hd, wd, bd, B, T, U, L, E, Y, blank, lattice_stream=side)
    torch.cuda.current_stream().wait_event(ev)
    valid = torch.from_numpy(c["ref"].valid).to(dev)
    assert torch.equal(nll1, nll2)
    for k, a, b in zip(("lse", "lpb", "lpy", "alpha", "beta"), ctx1, ctx2):
        if k in ("alpha", "beta"):
            a, b = a[valid], b[valid]
        assert torch.equal(a, b), k
    del keep
    assert _close_2e3(nll2.cpu().numpy(), c["ref"].nll)[1] <= 1.0


def test_fused_head_row_constants_with_a_device_scale(dev):
    """ops.rnnt_coef with gscale_dev: gscale * gscale_dev[0] -- the bits of the same product passed as gscale, and the reference's
    occupancies at that scale"""
    from emoasr_amd import ops
    c = _head_case(264, 64, True, True)
    B, T, U, blank, ref = c["B"], c["T"], c["U"], c["blank"], c["ref"]
    hd, wd, bd = c["h"].to(dev), c["w"].to(dev), c["bias"].to(dev)
    L, E, Y = _i32(c["labels"], dev), _i32(c["elens"], dev), _i32(c["ylens"], dev)
    ctx, nll = ops.rnnt_head_forward(hd, wd, bd, B, T, U, L, E, Y, blank)
    coef_h, ycol_h = ops.rnnt_coef(ctx, nll, L, E, Y, 0.125)
    coef_d, ycol_d = ops.rnnt_coef(ctx, nll, L, E, Y, 0.5, gscale_dev=torch.tensor([0.25], device=dev))
    assert torch.equal(coef_h, coef_d) and torch.equal(ycol_h, ycol_d)
    cf = coef_d.cpu().numpy().reshape(B, T, U, 4)
    gmax = float(np.abs(ref.dz).max()) / c["gs"] * 0.125
    for i, want in enumerate((ref.gb + ref.gy, ref.gb, ref.gy), 1):
        assert _worst(cf[..., i], want * 0.125, 3e-3 * gmax)[1] <= 1.0, i


# ---- the small kernels of csrc/rnnt.hip ------------------------------------------------------------------------------------------
_PLANTED = [0.0, 1e-5, -1e-5, 2.0 ** -8, -2.0 ** -8, 20.0, -20.0, 50.0, -50.0, 100.0, -100.0]


@pytest.mark.parametrize("J", [8, 12, 64, 520])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_joint_tanh(dev, dtype, J):
    """tanh(e[b,t] + g[b,u]) against float64 tanh of the rounded inputs.  bf16, J % 8 == 0: eight values per thread and
    1 - 2 * rcp(exp(2x) + 1) on the hardware units -- saturating to exactly +-1, finite for any sum; other J: tanhf per element.
    Bounds: f32 4 * 2^-23 absolute + 4e-7 relative (tanhf: a few ulp); bf16 2^-8 |ref| (output rounding) + 4 * 2^-23 (the
    absolute error of 1 - 2 * rcp(...) near 0, where the result is a difference of numbers near 1)"""
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(J)
    B, T, U = 2, 5, 3
    e = torch.randn(B, T, J, generator=g) * 1.5
    gg = torch.randn(B, U, J, generator=g) * 1.5
    # planted sums: as (x, 0) and as (x + 1.5, -1.5) -- exact in both dtypes for the large ones
    k = 0
    for x in _PLANTED:
        b, t, u, j = k % B, k % T, k % U, k % J
        e[b, t, j], gg[b, u, j] = x, 0.0
        k += 1
        b, t, u, j = k % B, (k + 2) % T, (k + 1) % U, (k + 3) % J
        if abs(x) >= 1 or x == 0.0:
            e[b, t, j], gg[b, u, j] = x + 1.5, -1.5
        k += 1
    e, gg = e.to(dtype), gg.to(dtype)
    x64 = e.double()[:, :, None, :] + gg.double()[:, None, :, :]
    assert sum(int((x64 == x).any()) for x in (0.0, 20.0, -20.0, 50.0, -50.0, 100.0, -100.0)) == 7
    ref = torch.tanh(x64).numpy()
    h = ops.joint_tanh(e.to(dev), gg.to(dev))
    assert h.shape == (B, T, U, J) and h.dtype == dtype
    got = h.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    bound = 4 * P23 + 4e-7 * np.abs(ref) if dtype == torch.float32 else P8 * np.abs(ref) + 4 * P23
    err, ratio = _worst(got, ref, bound)
    print(f"[measured] joint_tanh {str(dtype)[6:]} J={J}: err {err:.2e} {ratio:.2f} of bound")
    assert ratio <= 1.0, (err, ratio)
    if dtype == torch.bfloat16:
        big = (x64.abs() >= 20).numpy()
        assert big.sum() >= 12 and np.array_equal(got[big], np.sign(x64.numpy()[big]))
    assert (np.abs(got) <= 1.0).all()


@pytest.mark.parametrize("J", [8, 12, 64])
@pytest.mark.parametrize("T,U", [(1, 1), (3, 4), (4, 9), (5, 3), (9, 5), (1, 9), (4, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_joint_reduce(dev, dtype, T, U, J):
    """de = sum over u, dg = sum over t (f32 accumulation) against the float64 sums: n terms -> n * 2^-23 * sum |x|, bf16 output
    + 2^-8 |ref|.  T, U in {1, 3, 4, 5, 9}: the 4-term unroll of the 8-column kernel with every tail.  bf16: the 8-column kernel
    (16-byte aligned buffers, J % 8 == 0) and the element-wise kernel (the same data one element into a larger buffer) add in the
    same order: bit-identical."""
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(100 * T + 10 * U + J)
    B = 2
    d = torch.randn(B, T, U, J, generator=g).to(dtype)
    dd = d.to(dev)
    assert dd.data_ptr() % 16 == 0
    de, dg = ops.joint_reduce(dd)
    d64 = d.double()
    for name, got, ref, n, mag in (("de", de, d64.sum(2), U, d64.abs().sum(2)), ("dg", dg, d64.sum(1), T, d64.abs().sum(1))):
        bound = n * P23 * mag.numpy() + (P8 * ref.abs().numpy() if dtype == torch.bfloat16 else 0.0) + 1e-300
        err, ratio = _worst(got.float().cpu().numpy(), ref.numpy(), bound)
        print(f"[measured] joint_reduce {str(dtype)[6:]} T={T} U={U} J={J} {name}: err {err:.2e} {ratio:.2f} of bound")
        assert ratio <= 1.0, (name, err, ratio)
    if dtype == torch.bfloat16:
        flat = torch.zeros(d.numel() + 8, device=dev, dtype=dtype)
        assert flat.data_ptr() % 16 == 0
        off = flat[1:1 + d.numel()].view(B, T, U, J)
        off.copy_(dd)
        assert off.data_ptr() % 16 == 2 and off.is_contiguous()
        de2, dg2 = ops.joint_reduce(off)
        assert torch.equal(de, de2) and torch.equal(dg, dg2)


@pytest.mark.parametrize("V", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_argmax_rows(dev, dtype, V):
    """rows of a wider tensor (row stride > V); bf16 values from a coarse grid (many ties) and a planted tie of the maximum at
    columns 3 and 700: the lowest index wins, as numpy's argmax of the upcast; a row of -inf returns 0"""
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(V)
    M = 9
    wide = torch.randn(M, V + 24, generator=g)
    if dtype == torch.bfloat16:
        wide = ((wide * 4).round() / 4).clamp(max=1.0)     # a 0.25 grid cut at 1: every row's maximum is shared by many columns
    wide = wide.to(dtype)
    x = wide[:, 8:8 + V]
    if V > 700:
        x[2, 3] = x[2, 700] = 50.0
        x[3, 700] = x[3, 3] = 60.0
        x[4, 999] = 70.0
    x[5] = float("-inf")
    if V > 1:
        x[6, V - 1] = 80.0
        x[7, 0] = x[7, V - 1] = 80.0
    xd = wide.to(dev)[:, 8:8 + V]
    assert xd.stride(0) == V + 24
    got = ops.argmax_rows(xd).cpu().numpy()
    want = np.argmax(x.double().numpy(), axis=1)
    assert np.array_equal(got, want), (got, want)
    assert got[5] == 0
    if V > 700:
        assert got[2] == 3 and got[3] == 3 and got[4] == 999
    if dtype == torch.bfloat16 and V >= 255:
        xs = x.double().numpy()
        assert ((xs == xs.max(1, keepdims=True)).sum(1)[[0, 1, 8]] > 1).all()     # the grid did produce tied maxima


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 200])
def test_first_not_equal(dev, n):
    from emoasr_amd import ops
    value = 7

    def run(hits):
        x = torch.full((max(n, 1),), value, dtype=torch.int32)[:n].clone()
        for i, v in hits:
            x[i] = v
        xd = x.to(dev) if n else torch.full((1,), 99, dtype=torch.int32, device=dev)[:0]
        return ops.first_not_equal(xd, value).cpu().tolist()

    assert run([]) == [-1, value]
    for i in sorted({0, 63, 64, n - 1}):
        if 0 <= i < n:
            assert run([(i, 100 + i)]) == [i, 100 + i], i
    if n > 70:
        assert run([(70, 1), (5, 2)]) == [5, 2]
        assert run([(70, 1), (64 + 5, 2), (6, 3)]) == [6, 3]     # lane 5's second element against lane 6's first
