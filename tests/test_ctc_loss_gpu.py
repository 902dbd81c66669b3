"""The CTC loss at kernel level: csrc/ctc.hip (row log-sum-exp, emission gather, alpha / beta lattices, gradient rows -- dense and
over stacked micro-batches -- row arg-max and collapse) against the float64 reference of tests/ctc_ref.py (pinned on the CPU by
tests/test_ctc_ref_cpu.py), at the lattice and vocabulary edges where the kernels change path: frame counts around the 8-frame
prefetch chunk, one / two / three waves of lattice states, the full 1024-thread block, the 16-byte rows and the scalar fall-back
of both dtypes, the second trip of the 2048-column loop, LDS rows on both sides of 64 KiB, 64-frame passes of the collapse.

Bounds (none taken from the kernels under test):
  f32 lattice quantities   lse, lp, alpha, beta, nll: |got - ref64| <= max(4 * e32, 1e-4 * max(1, |ref|)).  e32 = the error of the
                           float32 evaluation of the same formulas (ctc_ref(dtype=float32), libm accuracy) on the same case; the
                           factor 4: the hardware exp2 / log2 units (a few ulp against libm's half) and another summation order;
                           1e-4: the suite's existing CTC tolerance (tests/test_ops_gpu.py::test_ctc).
  gradient                 max(4 * e32, 1e-4 * gs / 0.25) (the existing 1e-4 was taken at gs = 1/4); bf16: + 2^-8 |ref|, one ulp of
                           output rounding
  indices, zero rows, "bit-identical", NaN guards, refusals   exact

MEASURED on an MI355X, worst share of the bound per family (lattice quantities | gradient):
  prefetch chunk 0.00 | 0.03    waves 0.00 | 0.22    full block 0.02 | 0.25    long lattice 0.01 | 0.25    lengths past T 0.00 | 0.01
  vocabulary edges 0.00 | 0.75  unaligned 0.00 | 0.61  LDS rows 0.00 | 0.71    hard numerics 0.01 | 0.55   stacked 0.00 | 0.73
(the lattice errors sit at the float32 model's, 3e-7 .. 4e-6, far inside the suite's 1e-4; the gradient's largest shares are bf16
output rounding).  What the sweep exposed: row_lse returned NaN for a row whose -inf entry was the first element a thread saw with a
finite one behind it (exp(-inf - -inf)); test_minus_infinity_on_symbols_that_are_no_label[*-263] is the case."""
import numpy as np
import pytest
import torch

from tests.ctc_ref import ctc_greedy_ref, ctc_ref

pytestmark = pytest.mark.gpu

P8 = 2.0 ** -8
NAN = float("nan")


def _i32(a, dev):
    return torch.as_tensor(np.asarray(a)).to(torch.int32).to(dev)


def _labels(g, B, L, V, blank):
    lab = torch.randint(0, V - 1, (B, L), generator=g)
    return lab + (lab >= blank).long()     # any symbol but the blank


def _cyclic_labels(L, V, blank, repeats=()):
    """L labels without equal neighbours (feasible in L frames), except a forced repeat at each position of `repeats`"""
    syms = [v for v in range(V) if v != blank]
    lab = [syms[i % len(syms)] for i in range(L)]
    for i in repeats:
        if 0 < i < L:
            lab[i] = lab[i - 1]
    return torch.tensor(lab)


def _worst(got, ref, bound):
    """max of |got - ref| / bound over the entries where ref is finite; the others must be equal (+-inf in place)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]), "infinite entries differ"
    if not fin.any():
        return 0.0, 0.0
    assert np.isfinite(got[fin]).all(), "non-finite value where the reference is finite"
    err = np.abs(got[fin] - ref[fin])
    return float(err.max()), float((err / np.broadcast_to(bound, ref.shape)[fin]).max())


def _e32(m32, ref, sel=None):
    a, b = np.asarray(m32, np.float64), np.asarray(ref, np.float64)
    if sel is not None:
        a, b = a[sel], b[sel]
    fin = np.isfinite(b)
    return float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0


def _lattice_bound(e32, r):
    return np.maximum(4 * e32, 1e-4 * np.maximum(1.0, np.abs(np.where(np.isfinite(r), r, 0.0))))


def _dz_bound(e32, gs_total, ref_dz, dtype):
    bound = np.maximum(4 * e32, 1e-4 * gs_total / 0.25)
    return bound + P8 * np.abs(ref_dz) if dtype == torch.bfloat16 else bound


def _report(name, lines):
    print(f"[measured] ctc {name}: " + ", ".join(f"{k} err {e:.2e} (f32 model {m:.2e}) {r:.2f} of bound" for k, e, m, r in lines))
    for k, e, m, r in lines:
        assert r <= 1.0, (name, k, e, m, r)


_REF_CACHE = {}


def _refs(z, labels, elens, ylens, blank, gs_total, key=None):
    """(float64 reference, float32 model) on the rounded logits; with a key: computed once and shared by the runs that name it"""
    if key is None or key not in _REF_CACHE:
        args = (z.double().numpy(), np.asarray(labels), np.asarray(elens), np.asarray(ylens), blank)
        res = ctc_ref(*args, gs=gs_total), ctc_ref(*args, gs=gs_total, dtype=np.float32)
        if key is None:
            return res
        _REF_CACHE[key] = res
    return _REF_CACHE[key]


def _check(dev, name, z, labels, elens, ylens, blank, gs, gscale_dev=None, ld=None, ldg=None, offset=0, out_offset=0, key=None):
    """ops.row_lse + ops.ctc_forward + ops.ctc_grad on z (CPU tensor [B,T,V], f32 or bf16) against the float64 reference on the
    same rounded logits.  ld / ldg: row strides of the logits / of the gradient (pad columns NaN-filled: never read, never written);
    offset / out_offset: the tensors start that many elements into a larger buffer.  -> (lse, lp, alpha, beta, nll, dz, ref)"""
    from emoasr_amd import ops
    B, T, V = z.shape
    ld, ldg = ld or V, ldg or V
    gs_total = gs * (1.0 if gscale_dev is None else float(gscale_dev))
    ref, m32 = _refs(z, labels, elens, ylens, blank, gs_total, key)
    flat_in = torch.full((offset + B * T * ld + 8,), NAN, dtype=z.dtype)
    rows_in = flat_in[offset:offset + B * T * ld].view(B * T, ld)
    rows_in[:, :V] = z.reshape(B * T, V)
    flat_in = flat_in.to(dev)
    z2 = flat_in[offset:offset + B * T * ld].view(B * T, ld)[:, :V]
    zd = flat_in[offset:offset + B * T * ld].view(B, T, ld)[..., :V]
    assert zd.data_ptr() % 16 == (offset * z.element_size()) % 16
    L, E, Y = _i32(labels, dev), _i32(elens, dev), _i32(ylens, dev)
    lse = ops.row_lse(z2)
    lp, alpha, beta, nll = ops.ctc_forward(zd, lse, L, E, Y, blank)
    # NaN-filled, with a guard behind the last row: an unwritten row, a store into the pad columns or past the end all show
    n_out = B * T * ldg
    flat = torch.full((out_offset + n_out + 64,), NAN, device=dev, dtype=z.dtype)
    out = flat[out_offset:out_offset + n_out].view(B, T, ldg)[..., :V]
    gdev = None if gscale_dev is None else torch.tensor([gscale_dev], device=dev, dtype=torch.float32)
    dz = ops.ctc_grad(zd, lse, L, E, Y, blank, lp, alpha, beta, nll, gs, gscale_dev=gdev, out=out)
    assert dz.data_ptr() == out.data_ptr()
    assert bool(torch.isnan(flat[out_offset + n_out:]).all()) and bool(torch.isnan(flat[:out_offset]).all()), \
        f"{name}: the gradient kernel stored outside its rows"
    if ldg > V:
        assert bool(torch.isnan(flat[out_offset:out_offset + n_out].view(B * T, ldg)[:, V:]).all()), f"{name}: store into the pad columns"
    got = {"lse": lse.view(B, T).cpu().numpy(), "lp": lp.cpu().numpy(), "alpha": alpha.cpu().numpy(), "beta": beta.cpu().numpy(),
           "nll": nll.cpu().numpy()}
    frames = np.arange(T)[None, :] < np.minimum(np.asarray(elens), T)[:, None]     # [B,T]: the lattice rows the kernel writes
    lines = []
    for k in ("lse", "lp", "alpha", "beta", "nll"):
        sel = frames if k in ("alpha", "beta") else None      # (rows behind the utterance's end are left unwritten)
        r = getattr(ref, k) if sel is None else getattr(ref, k)[sel]
        gk = got[k] if sel is None else got[k][sel]
        e32 = _e32(getattr(m32, k), getattr(ref, k), sel)
        err, ratio = _worst(gk, r, _lattice_bound(e32, r))
        lines.append((k, err, e32, ratio))
    dzc = dz.float().cpu().numpy()
    assert np.isfinite(dzc).all(), f"{name}: gradient rows left unwritten (NaN fill) or non-finite"
    e32 = _e32(m32.dz, ref.dz)
    err, ratio = _worst(dzc, ref.dz, _dz_bound(e32, gs_total, ref.dz, z.dtype))
    lines.append(("dz", err, e32, ratio))
    _report(name, lines)
    dead = ~frames | ~np.isfinite(ref.nll)[:, None]
    assert (dzc[dead] == 0).all(), f"{name}: non-zero gradient behind the end of an utterance or for an infinite loss"
    return lse, lp, alpha, beta, nll, dz, ref


# ---- lattice geometry: f32, V = 8 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blank", [0, 3, 7])
def test_frame_counts_around_the_prefetch_chunk(dev, blank):
    """1, 2, 8, 9, 10, 16, 17, 18, 25 and 0 frames (the 8-frame chunk that starts at frame 1: none, one frame, one chunk - 1, exactly
    one, one + 1, ...), ragged, in ONE launch; among them rows without labels, rows whose frames are exactly labels + forced
    repeats, rows one frame short of that, a row of one repeated symbol and utterances without frames (with and without labels)"""
    g = torch.Generator().manual_seed(10 + blank)
    T, Lmax, V = 25, 3, 8
    a, b = [v for v in range(V) if v != blank][:2]
    #        0  1  2  3  4  5  6   7   8   9   10  11 12 13
    elens = [1, 1, 2, 2, 8, 9, 10, 16, 17, 18, 25, 0, 0, 5]
    ylens = [1, 0, 2, 2, 3, 3, 2, 3, 1, 3, 3, 0, 2, 3]
    B = len(elens)
    z = torch.randn(B, T, V, generator=g) * 2
    labels = _labels(g, B, Lmax, V, blank)
    labels[2, :2] = torch.tensor([a, b])      # two labels in two frames: exactly feasible
    labels[3, :2] = a                         # the same label twice needs a blank between: infeasible in two frames
    labels[5] = b                             # one repeated symbol (5 frames needed, 9 there)
    labels[13] = a                            # ... and in exactly 5 frames
    lse, lp, alpha, beta, nll, dz, ref = _check(dev, f"chunk blank={blank}", z, labels, elens, ylens, blank, 1.0 / B)
    fin = np.isfinite(ref.nll)
    assert fin.tolist() == [True, True, True, False, True, True, True, True, True, True, True, True, False, True]
    nl = nll.cpu().numpy()
    assert nl[11] == 0.0 and np.isposinf(nl[12]) and np.isposinf(nl[3])
    assert sorted(set(elens)) == [0, 1, 2, 5, 8, 9, 10, 16, 17, 18, 25]


@pytest.mark.parametrize("Lmax", [31, 32, 63, 64])
def test_state_counts_around_the_waves(dev, Lmax):
    """S = 63, 65, 127, 129 states: one wave not quite full, one state into the second, two waves, one state into the third; in the
    same block shorter label rows whose last state sits on and around the wave boundaries (Sb = 63, 65, 127 where they fit)"""
    g = torch.Generator().manual_seed(Lmax)
    T, V, blank = Lmax + 8, 8, 0
    ylens = [Lmax, min(Lmax, 31), min(Lmax, 32), min(Lmax, 63), Lmax - 1, 0]
    elens = [T, T - 1, T, T - 3, T, 5]
    B = len(ylens)
    z = torch.randn(B, T, V, generator=g) * 2
    labels = torch.stack([_cyclic_labels(Lmax, V, blank, repeats=(3 + b, 17, Lmax - 1 - b)) for b in range(B)])
    *_, ref = _check(dev, f"waves Lmax={Lmax}", z, labels, elens, ylens, blank, 1.0 / B)
    assert np.isfinite(ref.nll).all()
    assert {2 * y + 1 for y in ylens} >= {2 * Lmax + 1, 63}


def test_full_block_and_the_limit(dev):
    """Lmax = 511: S = 1023, all but one thread of the largest block own a state.  Lmax = 512 is refused before anything is launched."""
    from emoasr_amd import lib, ops
    g = torch.Generator().manual_seed(30)
    T, Lmax, V, blank = 520, 511, 8, 0
    ylens, elens = [511, 510, 32, 0], [520, 519, 520, 7]
    z = torch.randn(4, T, V, generator=g) * 2
    labels = torch.stack([_cyclic_labels(Lmax, V, blank, repeats=(5 + b, 200, 400, 509)) for b in range(4)])
    *_, ref = _check(dev, "S=1023", z, labels, elens, ylens, blank, 0.25)
    assert np.isfinite(ref.nll).all()
    Lmax = 512
    S = 2 * Lmax + 1
    z = torch.randn(1, 1, V, generator=g).to(dev)
    lab, one = torch.ones(1, Lmax, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    lse = torch.zeros(1, device=dev)
    with pytest.raises(lib.EmoasrHipError, match="exceeds 1024"):
        ops.ctc_forward(z, lse, lab, one, one, 0)
    bufs = [torch.full((1, 1, S), 7.0, device=dev) for _ in range(3)] + [torch.full((1,), 7.0, device=dev)]
    with pytest.raises(lib.EmoasrHipError, match="exceeds 1024"):
        lib.call("emoasr_ctc_forward", ops.dt(z), 1, 1, V, Lmax, ops._p(z), V, ops._p(lse), ops._p(lab), ops._p(one), ops._p(one), 0,
                 *[ops._p(b) for b in bufs], ops._stream())
    torch.cuda.synchronize()
    assert all(bool((b == 7.0).all()) for b in bufs)     # not even the gather ran


def test_long_lattice(dev):
    """T = 600, 81 states: the drift of the exp2 / log2 chain over hundreds of frames"""
    g = torch.Generator().manual_seed(40)
    B, T, Lmax, V = 2, 600, 40, 8
    z = torch.randn(B, T, V, generator=g) * 2
    _check(dev, "long", z, _labels(g, B, Lmax, V, 0), [600, 433], [40, 17], 0, 1.0)


def test_lengths_past_the_tensor_are_clamped(dev):
    """elens = T + 5 and T + 2: the lattice stops at the tables' last frame -- the reference's values, and the bits of elens = T"""
    g = torch.Generator().manual_seed(41)
    B, T, Lmax, V = 3, 10, 3, 8
    z = torch.randn(B, T, V, generator=g) * 2
    labels = _labels(g, B, Lmax, V, 0)
    res = _check(dev, "elens = T", z, labels, [10, 10, 10], [3, 1, 2], 0, 1.0)
    res5 = _check(dev, "elens past T", z, labels, [15, 10, 12], [3, 1, 2], 0, 1.0)
    for a, b in zip(res[:5], res5[:5]):
        assert torch.equal(a, b)
    assert torch.equal(res[5], res5[5])


# ---- vocabulary paths --------------------------------------------------------------------------------------------------------------
def _vocab_case(dtype, V, seed=0, T=6):
    g = torch.Generator().manual_seed(1000 * seed + V)
    B, Lmax = 2, 3
    blank = 1 if V > 2 else 0
    z = (torch.randn(B, T, V, generator=g) * 2).to(dtype)
    labels = _labels(g, B, Lmax, V, blank)
    tail = V // 8 * 8 if V % 8 else V - 2      # a label behind the last full group of 8 (in the last group when there is no tail)
    row0 = [0, V - 1, tail if tail != blank else V - 1]
    labels[0] = torch.tensor([v if v != blank else 1 - blank for v in row0])
    return z, labels, [T, T - 2], [3, 1], blank


_DT = [torch.float32, torch.bfloat16]
_DT_IDS = ["f32", "bf16"]


@pytest.mark.parametrize("V", [2, 7, 8, 9, 16, 2040, 2048, 2056, 4104])
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_vocabulary_edges(dev, dtype, V):
    """the 16-byte path (V, ld and ldg multiples of 8) up to the second and third trip of its 2048-column loop, and the scalar
    fall-back through V, through ld and through ldg; labels on column 0, on the last column and behind the last full group of 8;
    row strides larger than V on either side, different on the two sides; gscale * gscale_dev"""
    z, labels, elens, ylens, blank = _vocab_case(dtype, V)
    n = f"V={V} {_DT_IDS[_DT.index(dtype)]}"
    key = ("vocab", dtype, V)
    _check(dev, n + " packed", z, labels, elens, ylens, blank, 0.125, key=key)
    _check(dev, n + " ld=V+8 ldg=V+16", z, labels, elens, ylens, blank, 0.5, gscale_dev=0.25, ld=V + 8, ldg=V + 16, key=key)
    _check(dev, n + " ld=V+3", z, labels, elens, ylens, blank, 0.125, ld=V + 3, ldg=V + 8, key=key)
    _check(dev, n + " ldg=V+3", z, labels, elens, ylens, blank, 0.125, ld=V + 8, ldg=V + 3, key=key)


@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_unaligned_base_pointers_take_the_scalar_path(dev, dtype):
    """V = 16 with every stride a multiple of 8, but the logits (then the gradient) start one element into a larger buffer: the
    16-byte accesses would be misaligned; row_lse and the gradient kernel both fall back to scalar accesses"""
    z, labels, elens, ylens, blank = _vocab_case(dtype, 16, seed=2)
    n = f"V=16 {_DT_IDS[_DT.index(dtype)]}"
    key = ("unaligned", dtype)
    _check(dev, n + " logits + 1 element", z, labels, elens, ylens, blank, 0.5, offset=1, key=key)
    _check(dev, n + " gradient + 1 element", z, labels, elens, ylens, blank, 0.5, out_offset=1, key=key)
    _check(dev, n + " both + 1 element, ld = 24", z, labels, elens, ylens, blank, 0.5, offset=1, out_offset=1, ld=24, ldg=24, key=key)


@pytest.mark.parametrize("V", [16384, 16392, 40896])
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_lds_row_sizes(dev, dtype, V):
    """the softmax row in LDS: 64 KiB exactly, the first size that needs the raised limit, the largest accepted"""
    z, labels, elens, ylens, blank = _vocab_case(dtype, V, seed=3, T=4)
    z, labels = z[:1], labels[:1]
    _check(dev, f"V={V} {_DT_IDS[_DT.index(dtype)]}", z, labels, [4], [3], blank, 0.5)


def test_lds_row_limit_is_refused_before_launch(dev):
    from emoasr_amd import lib, ops
    V = 40904
    z, labels, elens, ylens, blank = _vocab_case(torch.float32, V, seed=3, T=4)
    zd = z[:1].to(dev)
    L, E, Y = _i32(labels[:1], dev), _i32([4], dev), _i32([3], dev)
    lse = ops.row_lse(zd.view(4, V))
    lp, alpha, beta, nll = ops.ctc_forward(zd, lse, L, E, Y, blank)
    out = torch.full_like(zd, 7.0)
    with pytest.raises(lib.EmoasrHipError, match="too large for an LDS row"):
        ops.ctc_grad(zd, lse, L, E, Y, blank, lp, alpha, beta, nll, 1.0, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- hard numerics -------------------------------------------------------------------------------------------------------------------
def test_peaked_rows(dev):
    """logits * 20: most occupancies underflow, the lattice sums are dominated by one term"""
    g = torch.Generator().manual_seed(50)
    B, T, Lmax, V = 3, 12, 3, 8
    z = torch.randn(B, T, V, generator=g) * 20
    _check(dev, "logits * 20", z, _labels(g, B, Lmax, V, 0), [12, 9, 4], [3, 2, 1], 0, 1.0 / B)


@pytest.mark.parametrize("V", [8, 263, 264])
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_minus_infinity_on_symbols_that_are_no_label(dev, dtype, V):
    """masked symbols: columns 0 and 5 (V > 256: and 256 .. 259) at -inf on every frame.  At V = 263 (scalar accesses) column 5 is
    the FIRST element its thread of the row log-sum-exp sees, and the finite column 261 follows; at V = 264 a whole 16-byte group of
    the f32 row is -inf.  Everything stays finite; the masked columns' gradient is exactly 0."""
    g = torch.Generator().manual_seed(60 + V)
    B, T, Lmax, blank = 2, 6, 3, 1
    masked = [0, 5] + ([256, 257, 258, 259] if V > 256 else [])
    z = torch.randn(B, T, V, generator=g) * 2
    z[..., masked] = float("-inf")
    free = torch.tensor([v for v in range(V) if v != blank and v not in masked])
    labels = free[torch.randint(0, len(free), (B, Lmax), generator=g)]
    *_, nll, dz, ref = _check(dev, f"-inf off the labels V={V} {_DT_IDS[_DT.index(dtype)]}", z.to(dtype), labels, [6, 4], [3, 2], blank, 0.5)
    assert bool(torch.isfinite(nll).all()) and np.isfinite(ref.nll).all()
    assert bool((dz[..., masked] == 0).all())


@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_minus_infinity_on_a_label(dev, dtype):
    """utterance 0: one of its labels at -inf on every frame -- no alignment: nll = +inf, gradient exactly 0; its neighbour, whose
    labels avoid the column, is untouched"""
    g = torch.Generator().manual_seed(70)
    B, T, Lmax, V, blank = 2, 6, 3, 8, 0
    z = torch.randn(B, T, V, generator=g) * 2
    z[0, :, 4] = float("-inf")
    labels = torch.tensor([[2, 4, 6], [1, 3, 5]])
    *_, nll, dz, ref = _check(dev, f"-inf on a label {_DT_IDS[_DT.index(dtype)]}", z.to(dtype), labels, [6, 6], [3, 3], blank, 0.5)
    assert bool(torch.isposinf(nll[0])) and bool(torch.isfinite(nll[1])) and bool((dz[0] == 0).all())


# ---- stacked micro-batches -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [16, 10], ids=["V16_vector", "V10_scalar"])
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_stacked_rows(dev, dtype, V):
    """ctc_forward_rows / ctc_grad_rows as engine._ctc_train_stacked drives them: three micro-batches of 2, 3 and 1 utterances with
    padded lengths 7, 12, 9 stacked into one [59, V] matrix, row0 / tpad per utterance, a gradient scale per micro-batch, the
    gradient written into the [:, :V] view of a [59, 64] buffer.  lp / alpha / beta / nll: the bits of the dense ctc_forward of each
    micro-batch (deterministic kernels, the same arithmetic).  The gradient: the reference with row_scale = uscale (not the dense
    kernel's bits: the occupancies are LDS float atomics, the blank receives L + 1 of them in any order); exactly 0 on the rows
    t in [elens, tpad); the columns V .. 63 and the guard behind the buffer stay NaN."""
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(80 + V)
    sizes, pads, scales = [2, 3, 1], [7, 12, 9], [0.5, 0.3, 0.2]
    Lmax, blank, Tmax, gscale = 3, 0, 12, 0.5
    elens = [7, 4, 12, 9, 1, 6]
    ylens = [3, 1, 2, 3, 0, 3]
    Btot, M = sum(sizes), sum(b * t for b, t in zip(sizes, pads))
    assert M == 59
    z2 = (torch.randn(M, V, generator=g) * 2).to(dtype)
    labels = _labels(g, Btot, Lmax, V, blank)
    row0, tpad, uscale, r = [], [], [], 0
    for Bk, Tk, sk in zip(sizes, pads, scales):
        row0 += [r + b * Tk for b in range(Bk)]
        tpad += [Tk] * Bk
        uscale += [sk / Bk] * Bk
        r += Bk * Tk
    # the reference sees the utterances as one dense batch padded to Tmax
    z3 = torch.zeros(Btot, Tmax, V, dtype=dtype)
    for b in range(Btot):
        z3[b, :tpad[b]] = z2[row0[b]:row0[b] + tpad[b]]
    us32 = np.asarray(uscale, np.float32).astype(np.float64)
    ref = ctc_ref(z3.double().numpy(), labels, elens, ylens, blank, gs=gscale, row_scale=us32)
    m32 = ctc_ref(z3.double().numpy(), labels, elens, ylens, blank, gs=gscale, row_scale=us32, dtype=np.float32)
    zd = z2.to(dev)
    L, E, Y = _i32(labels, dev), _i32(elens, dev), _i32(ylens, dev)
    row0_d = torch.tensor(row0, dtype=torch.int64, device=dev)
    tpad_d = torch.tensor(tpad, dtype=torch.int32, device=dev)
    us_d = torch.tensor(uscale, dtype=torch.float32, device=dev)
    lse = ops.row_lse(zd)
    lp, alpha, beta, nll = ops.ctc_forward_rows(zd, lse, L, E, Y, blank, row0_d, Tmax)
    flat = torch.full((M * 64 + 64,), NAN, device=dev, dtype=dtype)
    wide = flat[:M * 64].view(M, 64)
    out = ops.ctc_grad_rows(zd, lse, L, E, Y, blank, lp, alpha, beta, nll, gscale, row0_d, tpad_d, us_d, wide[:, :V])
    assert bool(torch.isnan(flat[M * 64:]).all()) and bool(torch.isnan(wide[:, V:]).all()), "store outside the gradient rows"
    # each micro-batch on its own, dense
    b0, r = 0, 0
    for Bk, Tk in zip(sizes, pads):
        zk = zd[r:r + Bk * Tk].view(Bk, Tk, V)
        lpk, ak, bk, nk = ops.ctc_forward(zk, lse[r:r + Bk * Tk], L[b0:b0 + Bk], E[b0:b0 + Bk], Y[b0:b0 + Bk], blank)
        assert torch.equal(nll[b0:b0 + Bk], nk)
        assert torch.equal(lp[b0:b0 + Bk, :Tk], lpk)
        for b in range(Bk):
            n = elens[b0 + b]
            assert torch.equal(alpha[b0 + b, :n], ak[b, :n]) and torch.equal(beta[b0 + b, :n], bk[b, :n])
        b0, r = b0 + Bk, r + Bk * Tk
    e32 = _e32(m32.nll, ref.nll)
    err, ratio = _worst(nll.cpu().numpy(), ref.nll, _lattice_bound(e32, ref.nll))
    lines = [("nll", err, e32, ratio)]
    outc = out.float().cpu().numpy()
    assert np.isfinite(outc).all(), "gradient rows left unwritten (NaN fill) or non-finite"
    got = np.zeros((Btot, Tmax, V))
    for b in range(Btot):
        got[b, :tpad[b]] = outc[row0[b]:row0[b] + tpad[b]]
        assert (outc[row0[b] + min(elens[b], tpad[b]):row0[b] + tpad[b]] == 0).all(), f"utterance {b}: padding rows not zero"
    e32 = _e32(m32.dz, ref.dz)
    err, ratio = _worst(got, ref.dz, _dz_bound(e32, gscale * np.asarray(uscale)[:, None, None], ref.dz, dtype))     # (a floor per utterance)
    lines.append(("dz", err, e32, ratio))
    _report(f"stacked V={V} {_DT_IDS[_DT.index(dtype)]}", lines)


# ---- greedy decoding --------------------------------------------------------------------------------------------------------------------
def _greedy_plan(T, V, blank, g):
    """per utterance the symbol every frame's arg-max must be, and elens.  Symbols at the 64-frame pass boundaries:
       0: equal across 63|64 and 127|128 (one run: collapses)      1: x blank x with the blank ON frame 63 / 127 (two symbols)
       2: x blank x with the blank on frame 64 / 128               3: elens = 64, a run that ends with the pass
       4: no frames                                                5: all blank"""
    syms = [v for v in range(V) if v != blank]
    rnd = lambda: [syms[int(i)] for i in torch.randint(0, len(syms), (T,), generator=g)]
    x = syms[-1]
    plan = [rnd() for _ in range(4)]
    for p in plan[:3]:                # some blanks and runs everywhere
        for t in range(0, T, 7):
            p[t] = blank
        for t in range(3, T, 11):
            p[t] = p[t - 1]
    for e in (63, 127):
        for off, p in ((0, plan[0]), (0, plan[1]), (1, plan[2])):
            for t in (e + off - 1, e + off, e + off + 1):
                if t < T:
                    p[t] = x
        if e < T:
            plan[1][e] = blank
        if e + 1 < T:
            plan[2][e + 1] = blank
    for t in range(60, min(64, T)):
        plan[3][t] = x
    plan += [rnd(), [blank] * T]
    return plan, [T, T, T, 64, 0, T]


def _ties(v, V):
    """columns above v that share its maximum: another lane of the wave, the same lane of later waves, the same thread's next trip"""
    return [u for u in (v + 3, v + 64, v + 128, v + 192, v + 256, v + 256 + 64, V - 1) if v < u < V]


@pytest.mark.parametrize("T", [63, 64, 65, 130])
@pytest.mark.parametrize("V", [3, 256, 257, 1000])
def test_greedy(dev, V, T):
    """arg-max with planted ties of the maximum (the lowest index wins: inside a wave, between waves, across the 256-column stride
    -- also with the lowest index in a LATER wave than a higher one) and the collapse over one, two and three 64-frame passes"""
    from emoasr_amd import ops
    for dtype in _DT:
        for blank in (0, V - 1):
            g = torch.Generator().manual_seed(V * 1000 + T + blank)
            plan, elens = _greedy_plan(T, V, blank, g)
            B, ld = len(plan), V + 5
            wide = torch.full((B, T, ld), NAN)
            z = ((torch.randn(B, T, V, generator=g) * 4).round() / 4).clamp(-2.0, 2.0)     # a 0.25 grid: ties below the maximum too
            for b in range(B):
                for t in range(T):
                    v = plan[b][t]
                    z[b, t, v] = 5.0
                    ties = _ties(v, V)
                    for u in ties[: (b + t) % (len(ties) + 1)]:
                        z[b, t, u] = 5.0
            # the lowest index in a later wave than a higher one: columns 100 (wave 1) and 300 (wave 0 of the second trip)
            if V > 300 and blank != 100:
                z[0, 1, :] = -1.0
                z[0, 1, 300] = z[0, 1, 100] = 5.0
                plan[0][1] = 100
            wide[..., :V] = z
            zd = wide.to(dtype).to(dev)[..., :V]
            best, hyp, hyplen = ops.ctc_greedy(zd, _i32(elens, dev), blank)
            want_best, want = ctc_greedy_ref(zd.float().cpu().numpy(), elens, blank)
            assert want_best.tolist() == plan, "the planted maxima are not the reference's arg-max"
            assert np.array_equal(best.cpu().numpy(), want_best), (str(dtype), blank)
            lens = hyplen.cpu().tolist()
            assert lens == [len(h) for h in want], (lens, [len(h) for h in want])
            for b in range(B):
                assert hyp[b, :lens[b]].cpu().tolist() == want[b], (str(dtype), blank, b)
            assert lens[4] == 0 and lens[5] == 0
            x = [v for v in range(V) if v != blank][-1]
            if T > 64:      # around the pass boundary: one x for the run, two for x blank x
                def count(b, lo, hi):
                    idx = [t for t in range(lo, min(hi, T))]
                    seq = [plan[b][t] for t in idx]
                    return sum(1 for i, v in enumerate(seq) if v == x and (i == 0 or seq[i - 1] != x))
                assert count(0, 62, 66) == 1 and count(1, 62, 66) == 2
                if T > 66:
                    assert count(2, 63, 67) == 2
