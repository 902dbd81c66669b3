"""tests/ctc_ref.py (the numpy reference of the CTC / cross-entropy kernel tests) pinned in float64 at 1e-10: nll against the
enumeration of every alignment, nll and the gradient against torch's CTC loss + autograd on float64 CPU tensors, the lattice
tables through "alpha and beta meet at every frame", and the two cross-entropy references against autograd of a restatement
with torch.log_softmax and the label-smoothed one-hot."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.ctc_ref import ctc_greedy_ref, ctc_ref, lsm_ref, soft_ce_ref

TOL = 1e-10


def _collapse(path, blank):
    out, prev = [], -1
    for v in path:
        if v != prev and v != blank:
            out.append(v)
        prev = v
    return out


def _enumerate_nll(z, label, blank):
    """-log of the total probability of every frame-level path that collapses to `label`"""
    T, V = z.shape
    p = np.exp(z - np.log(np.exp(z).sum(-1, keepdims=True)))
    tot = 0.0
    for path in itertools.product(range(V), repeat=T):
        if _collapse(path, blank) == list(label):
            tot += float(np.prod([p[t, v] for t, v in enumerate(path)]))
    return -np.log(tot) if tot > 0 else np.inf


@pytest.mark.parametrize("blank", [0, 1, 2])
def test_nll_against_the_enumeration_of_every_alignment(blank):
    rng = np.random.default_rng(blank)
    V = 3
    syms = [v for v in range(V) if v != blank]
    n = 0
    for T in range(1, 6):
        for L in range(0, 3):
            for label in itertools.product(syms, repeat=L):
                z = rng.standard_normal((1, T, V)) * 2
                lab = np.zeros((1, 2), np.int64)
                lab[0, :L] = label
                r = ctc_ref(z, lab, [T], [L], blank)
                want = _enumerate_nll(z[0], label, blank)
                if np.isinf(want):
                    assert np.isposinf(r.nll[0]) and (r.dz == 0).all(), (T, label)
                else:
                    assert abs(r.nll[0] - want) < TOL, (T, label, r.nll[0], want)
                n += 1
    assert n == 5 * (1 + 2 + 4)


# name: (T, V, blank, elens, ylens, labels | None = random without the blank)
CASES = {
    "ragged": (9, 6, 0, [9, 7, 4, 1, 5], [4, 2, 0, 1, 3], None),
    "blank_middle": (8, 7, 3, [8, 6, 8], [3, 3, 1], None),
    "blank_last": (8, 5, 4, [8, 5, 2], [4, 2, 2], None),
    "repeated_labels": (9, 5, 0, [9, 9, 7], [4, 3, 4], [[2, 2, 3, 3], [1, 1, 1, 0], [4, 2, 2, 4]]),
    "one_symbol_row": (10, 4, 1, [10, 7], [5, 4], [[3, 3, 3, 3, 3], [2, 2, 2, 2, 0]]),
    "no_labels": (5, 4, 2, [5, 1, 3], [0, 0, 0], None),
    "infeasible": (6, 5, 0, [6, 2, 2, 4], [3, 3, 2, 3], [[1, 2, 3], [1, 2, 3], [4, 4, 0], [2, 2, 2]]),   # rows 1-3: too few frames
    "exactly_feasible": (7, 5, 0, [6, 5, 3], [4, 3, 3], [[1, 1, 2, 2], [3, 3, 3, 0], [1, 2, 3, 0]]),    # frames = labels + repeats
    "elens_past_T": (6, 5, 0, [9, 6, 7], [2, 3, 1], None),
}


def _case(name):
    T, V, blank, elens, ylens, labels = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    B, Lmax = len(elens), max(max(ylens), 1)
    z = torch.randn(B, T, V, generator=g, dtype=torch.float64) * 2
    if labels is None:
        labels = torch.randint(0, V - 1, (B, Lmax), generator=g)
        labels = labels + (labels >= blank).long()
    else:
        labels = torch.tensor(labels)
    return z, labels, torch.tensor(elens), torch.tensor(ylens), blank


@pytest.mark.parametrize("name", sorted(CASES))
def test_float64_reference_against_torch_on_the_cpu(name):
    z, labels, elens, ylens, blank = _case(name)
    B, T, V = z.shape
    gs = 0.37
    scale = torch.linspace(0.5, 1.5, B, dtype=torch.float64)
    zr = z.clone().requires_grad_(True)
    lsm = zr.log_softmax(-1).transpose(0, 1)
    ec = elens.clamp(max=T)
    nll_t = F.ctc_loss(lsm, labels, ec, ylens, blank=blank, reduction="none", zero_infinity=False).detach()
    per = F.ctc_loss(lsm, labels, ec, ylens, blank=blank, reduction="none", zero_infinity=True)
    (per * scale).sum().mul(gs).backward()
    r = ctc_ref(z.numpy(), labels.numpy(), elens.numpy(), ylens.numpy(), blank, gs=gs, row_scale=scale.numpy())
    assert r.nll.dtype == np.float64 and r.dz.dtype == np.float64
    fin = np.isfinite(nll_t.numpy())
    assert np.array_equal(np.isfinite(r.nll), fin) and np.isposinf(r.nll[~fin]).all()
    assert np.abs(r.nll[fin] - nll_t.numpy()[fin]).max() < TOL
    assert np.abs(r.dz - zr.grad.numpy()).max() < TOL
    assert (r.dz[~fin] == 0).all()
    if name == "infeasible":
        assert list(fin) == [True, False, False, False]
    if name == "exactly_feasible":
        assert fin.all()
    # reduction="sum" is the sum of the rows
    tot = F.ctc_loss(lsm.detach(), labels, ec, ylens, blank=blank, reduction="sum", zero_infinity=True)
    assert abs(float(tot) - r.nll[fin].sum()) < TOL * max(1.0, float(tot))
    assert np.abs(r.lse - torch.logsumexp(z, -1).numpy()).max() < TOL
    lpn = z.log_softmax(-1).numpy()
    for b in range(B):
        Tb, L = min(int(elens[b]), T), int(ylens[b])
        Sb = 2 * L + 1
        assert r.valid[b].sum() == Tb * Sb and r.valid[b, :Tb, :Sb].all()
        ext = [blank if s % 2 == 0 else int(labels[b, s // 2]) for s in range(Sb)]
        assert np.abs(r.lp[b, :Tb, :Sb] - lpn[b, :Tb][:, ext]).max() < TOL
        assert (r.dz[b, Tb:] == 0).all()
        if not fin[b]:
            continue
        # alpha and beta meet: the path mass through the states of any frame is the total
        with np.errstate(invalid="ignore"):
            post = r.alpha[b, :Tb, :Sb] + r.beta[b, :Tb, :Sb] - r.lp[b, :Tb, :Sb]
        assert np.abs(np.log(np.exp(post + r.nll[b]).sum(-1))).max() < TOL, b
        # every alpha row: the total of the sub-problem that ends there (frames 0..t, the label prefix of state s)
        for t in range(Tb):
            for s in range(Sb):
                k = (s + 1) // 2      # labels consumed in state s
                sub = F.ctc_loss(lsm.detach()[:t + 1, b:b + 1], labels[b:b + 1, :max(k, 1)], torch.tensor([t + 1]), torch.tensor([k]),
                                 blank=blank, reduction="none", zero_infinity=False)
                # the sub-problem ends on label k (state 2k - 1) or on the blank behind it (state 2k): the pair's sum is its total;
                # without labels it is state 0 alone
                if s % 2 == 1 or s == 0:
                    a = r.alpha[b, t, s]
                    if s % 2 == 1:
                        a = np.logaddexp(a, r.alpha[b, t, s + 1])
                    want = -float(sub[0])
                    assert (np.isneginf(a) and np.isneginf(want)) or abs(a - want) < TOL, (b, t, s)
    assert np.abs(r.dz.sum(-1)).max() < TOL     # softmax and occupancies both sum to 1
    for k in ("lp", "alpha", "beta"):
        assert np.isneginf(getattr(r, k)[~r.valid]).all()


def test_utterances_without_frames_and_the_float32_model():
    z, labels, elens, ylens, blank = _case("ragged")
    e0 = elens.clone()
    e0[1], e0[2] = 0, 0          # ylens 2 and 0
    r = ctc_ref(z.numpy(), labels.numpy(), e0.numpy(), ylens.numpy(), blank, gs=0.25)
    full = ctc_ref(z.numpy(), labels.numpy(), elens.numpy(), ylens.numpy(), blank, gs=0.25)
    assert np.isposinf(r.nll[1]) and r.nll[2] == 0.0
    assert (r.dz[1:3] == 0).all() and not r.valid[1:3].any()
    keep = [0, 3, 4]
    assert np.array_equal(r.nll[keep], full.nll[keep]) and np.array_equal(r.dz[keep], full.dz[keep])
    r32 = ctc_ref(z.numpy(), labels.numpy(), e0.numpy(), ylens.numpy(), blank, gs=0.25, dtype=np.float32)
    for k in ("lse", "lp", "alpha", "beta", "nll", "dz"):
        a, b = getattr(r32, k), getattr(r, k)
        assert a.dtype == np.float32, k
        fin = np.isfinite(b)
        assert np.array_equal(a[~fin], b[~fin].astype(np.float32)), k
        err = np.abs(a[fin] - b[fin]).max()
        assert 0 < err < 2e-5, (k, err)     # (it IS float32: not bit-equal to the reference)
    assert np.array_equal(r32.valid, r.valid)


def test_emissions_of_minus_infinity():
    """a symbol that is no label at -inf: everything stays finite; a label at -inf on every frame: no alignment"""
    z, labels, elens, ylens, blank = _case("blank_middle")
    zn = z.numpy().copy()
    used = {int(v) for b in range(3) for v in labels[b, :int(ylens[b])]} | {blank}
    free = [v for v in range(zn.shape[-1]) if v not in used]
    assert free
    zn[..., free[0]] = -np.inf
    r = ctc_ref(zn, labels.numpy(), elens.numpy(), ylens.numpy(), blank)
    assert np.isfinite(r.nll).all() and np.isfinite(r.dz).all() and (r.dz[..., free[0]] == 0).all()
    zn = z.numpy().copy()
    zn[0, :, int(labels[0, 1])] = -np.inf
    r = ctc_ref(zn, labels.numpy(), elens.numpy(), ylens.numpy(), blank)
    assert np.isposinf(r.nll[0]) and (r.dz[0] == 0).all() and np.isfinite(r.nll[1:]).all() and not np.isnan(r.dz).any()


def test_greedy_reference():
    z = np.zeros((2, 7, 4))
    for t, v in enumerate([1, 1, 0, 1, 2, 2, 3]):
        z[0, t, v] = 1.0
    z[1, :, 3] = 1.0
    z[1, 2, 1] = z[1, 2, 2] = 5.0     # a tie: the first maximum
    best, hyps = ctc_greedy_ref(z, [7, 9], 0)
    assert best[0].tolist() == [1, 1, 0, 1, 2, 2, 3] and hyps[0] == [1, 1, 2, 3]
    assert best[1].tolist() == [3, 3, 1, 3, 3, 3, 3] and hyps[1] == [3, 1, 3]
    assert ctc_greedy_ref(z, [3, 0], 3)[1] == [[1, 0], []]
    assert ctc_greedy_ref(z, [7, 7], 3)[1][1] == [1]


def _smoothed_onehot(V, y, eps):
    q = torch.full((V,), eps / (V - 1), dtype=torch.float64)
    q[y] = 1 - eps
    return q


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("V", [2, 7])
def test_label_smoothing_reference_against_autograd(V, eps):
    g = torch.Generator().manual_seed(V)
    M, gs = 5, 0.7
    z = torch.randn(M, V, generator=g, dtype=torch.float64) * 2
    labels = torch.tensor([0, V - 1, 1, 0, V - 1])
    w = torch.tensor([0.5, 1.0, 0.0, 0.25, 2.0], dtype=torch.float64)
    zr = z.clone().requires_grad_(True)
    lp = torch.log_softmax(zr, -1)
    loss = torch.stack([-w[m] * (_smoothed_onehot(V, int(labels[m]), eps) * lp[m]).sum() for m in range(M)])
    (loss.sum() * gs).backward()
    r = lsm_ref(z.numpy(), labels.numpy(), w.numpy(), eps, gs=gs)
    assert np.abs(r.loss - loss.detach().numpy()).max() < TOL
    assert np.abs(r.grad - zr.grad.numpy()).max() < TOL
    assert r.loss[2] == 0 and (r.grad[2] == 0).all()
    assert (r.mag >= np.abs(r.loss) - TOL).all()
    r32 = lsm_ref(z.numpy(), labels.numpy(), w.numpy(), eps, gs=gs, dtype=np.float32)
    assert r32.loss.dtype == np.float32 and r32.grad.dtype == np.float32
    assert np.abs(r32.loss - r.loss).max() < 1e-5 and np.abs(r32.grad - r.grad).max() < 1e-5


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("with_lrow", [False, True], ids=["all_rows", "lrow"])
def test_soft_cross_entropy_reference_against_autograd(eps, with_lrow):
    g = torch.Generator().manual_seed(3 + with_lrow)
    V, gs = 6, 1.3
    M = 8 if with_lrow else 6
    z = torch.randn(M, V, generator=g, dtype=torch.float64) * 2
    soft = torch.rand(3, V, generator=g, dtype=torch.float64)
    soft[0] /= soft[0].sum()                       # one proper distribution; rows 1 and 2 sum to something else
    #          soft only, hard only, both, neither, both (repeated source), soft only
    src = torch.tensor([2, -1, 0, -1, 2, 1])
    hard = torch.tensor([-1, 0, V - 1, -1, 3, -1])
    ws = torch.tensor([0.5, 9.0, 1.0, 9.0, 0.3, 2.0], dtype=torch.float64)
    wh = torch.tensor([9.0, 1.5, 0.5, 9.0, 0.7, 9.0], dtype=torch.float64)
    lrow = torch.tensor([6, 1, 4]) if with_lrow else None
    rows = lrow if with_lrow else torch.arange(M)
    R = len(rows)
    src, hard, ws, wh = src[:R], hard[:R], ws[:R], wh[:R]
    zr = z.clone().requires_grad_(True)
    lp = torch.log_softmax(zr, -1)
    per = []
    for r in range(R):
        l = lp[int(rows[r])]
        tot = torch.zeros((), dtype=torch.float64)
        if src[r] >= 0:
            tot = tot + ws[r] * (soft[int(src[r])] * l).sum()
        if hard[r] >= 0:
            tot = tot + wh[r] * (_smoothed_onehot(V, int(hard[r]), eps) * l).sum()
        per.append(-tot)
    per = torch.stack(per)
    (per.sum() * gs).backward()
    ref = soft_ce_ref(z.numpy(), soft.numpy(), src.numpy(), hard.numpy(), ws.numpy(), wh.numpy(), eps, gs=gs,
                      lrow=None if lrow is None else lrow.numpy())
    assert np.abs(ref.loss - per.detach().numpy()).max() < TOL
    assert np.abs(ref.grad - zr.grad.numpy()).max() < TOL
    if with_lrow:
        untouched = [m for m in range(M) if m not in lrow.tolist()]
        assert (ref.grad[untouched] == 0).all() and np.abs(ref.grad[lrow.numpy()]).min() > 0
    else:
        assert ref.loss[3] == 0 and (ref.grad[3] == 0).all()
    assert (ref.mag >= np.abs(ref.loss) - TOL).all()
    # soft only / hard only through the None arguments
    only_h = soft_ce_ref(z.numpy(), None, None, hard.numpy(), None, wh.numpy(), eps, gs=gs, lrow=None if lrow is None else lrow.numpy())
    want = lsm_ref(z.numpy()[rows.numpy()], np.maximum(hard.numpy(), 0), np.where(hard.numpy() >= 0, wh.numpy(), 0.0), eps, gs=gs)
    assert np.abs(only_h.loss - want.loss).max() < TOL
    assert np.abs(only_h.grad[rows.numpy()] - want.grad).max() < TOL
    r32 = soft_ce_ref(z.numpy(), soft.numpy(), src.numpy(), hard.numpy(), ws.numpy(), wh.numpy(), eps, gs=gs,
                      lrow=None if lrow is None else lrow.numpy(), dtype=np.float32)
    assert r32.loss.dtype == np.float32 and np.abs(r32.loss - ref.loss).max() < 2e-5 and np.abs(r32.grad - ref.grad).max() < 2e-5
