"""tests/rnnt_ref.py (the vectorised float64 reference of the transducer kernel tests) pinned against oracle/rnnt.py::rnnt_nll --
itself pinned by path enumeration in tests/test_oracle_rnnt.py -- and its autograd gradient, both in float64."""
import numpy as np
import pytest
import torch

from oracle import rnnt as orn
from tests.rnnt_ref import rnnt_ref

# (B, T, U, V, blank, elens, ylens, labels | None = random)
CASES = {
    "ragged": (4, 7, 5, 6, 0, [7, 5, 3, 1], [4, 2, 0, 3], None),
    "one_frame": (2, 1, 4, 5, 2, [1, 1], [3, 0], None),
    "no_labels": (3, 4, 3, 4, 3, [4, 1, 2], [0, 0, 0], None),
    "repeated_label_last_blank": (2, 6, 5, 7, 6, [6, 4], [4, 3], [[2, 2, 2, 2], [5, 5, 5, 0]]),
    "label_equals_blank": (2, 3, 3, 4, 1, [3, 2], [2, 1], [[1, 3], [1, 0]]),
    "elens_past_T": (2, 5, 3, 5, 0, [9, 5], [2, 1], None),
}


def _case(name):
    B, T, U, V, blank, elens, ylens, labels = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    z = torch.randn(B, T, U, V, generator=g, dtype=torch.float64) * 2
    if labels is None:
        labels = torch.randint(0, V - 1, (B, U - 1), generator=g)
        labels = labels + (labels >= blank).long()     # any symbol but the blank
    else:
        labels = torch.tensor(labels)
    return z, labels, torch.tensor(elens), torch.tensor(ylens), blank


@pytest.mark.parametrize("name", sorted(CASES))
def test_float64_reference_against_the_oracle(name):
    z, labels, elens, ylens, blank = _case(name)
    B, T, U, V = z.shape
    gs = 0.37
    zr = z.clone().requires_grad_(True)
    lp = torch.log_softmax(zr, -1)
    nll_o = orn.rnnt_nll(lp, labels, elens.clamp(max=T), ylens, blank)
    (nll_o.sum() * gs).backward()
    r = rnnt_ref(z.numpy(), labels.numpy(), elens.numpy(), ylens.numpy(), blank, gs=gs)
    assert r.nll.dtype == np.float64 and r.dz.dtype == np.float64
    assert np.abs(r.nll - nll_o.detach().numpy()).max() < 1e-10
    assert np.abs(r.dz - zr.grad.numpy()).max() < 1e-10
    lpn = lp.detach().numpy()
    assert np.abs(r.lse - torch.logsumexp(z, -1).numpy()).max() < 1e-10
    assert np.abs(r.lpb - lpn[..., blank]).max() < 1e-10
    for b in range(B):
        Tb, Ub = min(int(elens[b]), T), int(ylens[b])
        for u in range(U):
            if u < Ub:
                assert np.abs(r.lpy[b, :, u] - lpn[b, :, u, int(labels[b, u])]).max() < 1e-10
            else:
                assert np.isneginf(r.lpy[b, :, u]).all()
        assert r.valid[b].sum() == Tb * (Ub + 1) and r.valid[b, :Tb, :Ub + 1].all()
        # the two ends of the lattice carry the total
        assert abs(r.alpha[b, Tb - 1, Ub] + r.lpb[b, Tb - 1, Ub] + r.nll[b]) < 1e-10
        assert abs(r.beta[b, 0, 0] + r.nll[b]) < 1e-10
        assert r.alpha[b, 0, 0] == 0.0
        # every alpha cell: the oracle's total of the sub-lattice that ends there
        for t in range(Tb):
            for u in range(Ub + 1):
                sub = orn.rnnt_nll(lp.detach()[b:b + 1], labels[b:b + 1], [t + 1], [u], blank)
                assert abs(r.alpha[b, t, u] + r.lpb[b, t, u] + float(sub[0])) < 1e-10, (b, t, u)
        # every anti-diagonal that crosses the whole lattice carries the total as well: sum over its cells of the path mass
        # through the cell.  With alpha pinned above this pins beta.
        occ = r.alpha[b, :Tb, :Ub + 1] + r.beta[b, :Tb, :Ub + 1]
        tt, uu = np.meshgrid(np.arange(Tb), np.arange(Ub + 1), indexing="ij")
        for d in range(Tb + Ub):
            assert abs(np.log(np.exp(occ[tt + uu == d] + r.nll[b]).sum())) < 1e-10, (b, d)
    assert (r.dz[~r.valid] == 0).all()
    assert np.isneginf(r.alpha[~r.valid]).all() and np.isneginf(r.beta[~r.valid]).all()


def test_empty_utterance_and_the_float32_model():
    z, labels, elens, ylens, blank = _case("ragged")
    elens0 = elens.clone()
    elens0[1] = 0
    r = rnnt_ref(z.numpy(), labels.numpy(), elens0.numpy(), ylens.numpy(), blank, gs=0.25)
    full = rnnt_ref(z.numpy(), labels.numpy(), elens.numpy(), ylens.numpy(), blank, gs=0.25)
    assert np.isposinf(r.nll[1]) and (r.dz[1] == 0).all() and not r.valid[1].any()
    keep = [0, 2, 3]
    assert np.array_equal(r.nll[keep], full.nll[keep]) and np.array_equal(r.dz[keep], full.dz[keep])   # neighbours untouched
    # the float32 evaluation: same quantities, float32 throughout, within float32 rounding of the reference
    r32 = rnnt_ref(z.numpy(), labels.numpy(), elens0.numpy(), ylens.numpy(), blank, gs=0.25, dtype=np.float32)
    for k in ("lse", "lpb", "lpy", "alpha", "beta", "nll", "dz"):
        a, b = getattr(r32, k), getattr(r, k)
        assert a.dtype == np.float32, k
        fin = np.isfinite(b)
        assert np.array_equal(a[~fin], b[~fin].astype(np.float32)), k
        err = np.abs(a[fin] - b[fin]).max()
        assert 0 < err < 2e-5, (k, err)     # (it IS float32: not bit-equal to the reference)
    assert np.array_equal(r32.valid, r.valid)


def test_reference_is_fast_enough_for_a_sweep():
    """the largest lattice of the GPU sweep (tests/test_rnnt_loss_gpu.py) well under a second -- oracle/rnnt.py's loop over cells
    with autograd takes seconds there"""
    import time
    rng = np.random.default_rng(0)
    z = rng.standard_normal((2, 120, 41, 8)) * 2
    labels = rng.integers(1, 8, (2, 40))
    t0 = time.perf_counter()
    r = rnnt_ref(z, labels, [120, 90], [40, 17], 0, gs=1.0)
    dt = time.perf_counter() - t0
    assert np.isfinite(r.nll).all()
    assert dt < 1.0, dt
