"""recurrence.lstm_stack_fwd / lstm_stack_bwd against the loop they replace, written out here as the callers had it: lstm_layer_fwd +
scale_dropout per layer, then the mirrored lstm_layer_bwd loop.  Nothing but the call structure differs, so every output, every
stashed tensor and every accumulated gradient is compared with torch.equal.

Two layers, E = 16, H = 32, B = 3: U = 5 in bf16 is the cooperative recurrence, U = 5 in f32 the per-position chain, U = 1 in bf16
the chain again (the cooperative launch needs U > 1), which with a state is the searches' single step."""
import pytest
import torch

pytestmark = pytest.mark.gpu
NL, E, H, B = 2, 16, 32, 3
CASES = {"coop_bf16": (5, torch.bfloat16), "chain_f32": (5, torch.float32), "step_bf16": (1, torch.bfloat16)}


def _loop_fwd(x, W, seeds, state, p):
    from emoasr_amd import ops
    from emoasr_amd.recurrence import lstm_layer_fwd
    U = x.shape[0]
    layers, new_h, new_c = [], [], []
    for l, (w_ih, w_hh, bias) in enumerate(W):
        h0, c0 = (state[0][l], state[1][l]) if state is not None else (None, None)
        hseq, cseq, gact = lstm_layer_fwd(x, w_ih, w_hh, bias, h0, c0)
        new_h.append(hseq[U - 1])
        new_c.append(cseq[U - 1])
        y = ops.scale_dropout(hseq, 1.0, p, seeds[l]) if p > 0 else hseq
        layers.append((x, hseq, cseq, gact, seeds[l], h0, c0))
        x = y
    return x, (new_h, new_c), layers


def _loop_bwd(dy, layers, W, G, p):
    from emoasr_amd import ops
    from emoasr_amd.recurrence import lstm_layer_bwd
    for l in reversed(range(len(W))):
        x_in, hseq, cseq, gact, s_do, h0, c0 = layers[l]
        dh_seq = ops.scale_dropout(dy, 1.0, p, s_do) if p > 0 else dy
        dy = lstm_layer_bwd(dh_seq, x_in, hseq, cseq, gact, h0, c0, W[l][0], W[l][1], *G[l])
    return dy


@pytest.mark.parametrize("b_hh", [True, False], ids=["g_b_hh", "no_g_b_hh"])
@pytest.mark.parametrize("p", [0.0, 0.25], ids=["p0", "p25"])
@pytest.mark.parametrize("with_state", [True, False], ids=["h0c0", "zero_state"])
@pytest.mark.parametrize("case", list(CASES))
def test_stack_is_the_loop(dev, case, with_state, p, b_hh):
    from emoasr_amd import ops
    from emoasr_amd.recurrence import lstm_stack_bwd, lstm_stack_fwd
    U, dtype = CASES[case]
    g = torch.Generator().manual_seed(5)
    rnd = lambda *shape, dt=dtype, s=1.0: (torch.randn(*shape, generator=g) * s).to(dev).to(dt)
    W = [(rnd(4 * H, E if l == 0 else H, s=0.3), rnd(4 * H, H, s=0.3), rnd(4 * H, dt=torch.float32, s=0.3)) for l in range(NL)]
    x, dy = rnd(U, B, E), rnd(U, B, H)
    state = ([rnd(B, H) for _ in range(NL)], [rnd(B, H, dt=torch.float32) for _ in range(NL)]) if with_state else None
    seeds = [0x5EED + 7010 + l for l in range(NL)]
    g0 = [(rnd(4 * H, E if l == 0 else H, dt=torch.float32), rnd(4 * H, H, dt=torch.float32), rnd(4 * H, dt=torch.float32),
           rnd(4 * H, dt=torch.float32) if b_hh else None) for l in range(NL)]      # (nonzero: the gradients are accumulated into)
    clone = lambda G: [tuple(None if t is None else t.clone() for t in gl) for gl in G]
    with ops.stream_scope(False):
        assert ops.lstm_seq_supported(x, B, H) == (dtype == torch.bfloat16)
        y_ref, (h_ref, c_ref), lay_ref = _loop_fwd(x, W, seeds, state, p)
        G_ref = clone(g0)
        dx_ref = _loop_bwd(dy, lay_ref, W, G_ref, p)

        spec = [(*W[l], seeds[l], state[0][l] if state else None, state[1][l] if state else None) for l in range(NL)]
        y, (hs, cs), recs = lstm_stack_fwd(x, iter(spec), p, True)
        G = clone(g0)
        dx = lstm_stack_bwd(dy, recs, G, p)
        y2, _, none = lstm_stack_fwd(x, spec, p, False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(y2, y_ref)
    assert torch.equal(y, y_ref) and torch.equal(dx, dx_ref) and dx.shape == (U, B, E)
    assert len(recs) == len(hs) == len(cs) == NL
    for l in range(NL):
        assert torch.equal(hs[l], h_ref[l]) and torch.equal(cs[l], c_ref[l])
        r = recs[l]
        for got, want in zip((r.x, r.hseq, r.cseq, r.gact), lay_ref[l][:4]):
            assert torch.equal(got, want)
        assert r.s_do == seeds[l] and r.w_ih is W[l][0] and r.w_hh is W[l][1]
        assert (r.h0 is None and r.c0 is None) if state is None else (r.h0 is state[0][l] and r.c0 is state[1][l])
        for got, want in zip(G[l], G_ref[l]):
            assert (got is None and want is None) or torch.equal(got, want)
        assert not torch.equal(G[l][0], g0[l][0])      # (and something was accumulated)
        if p > 0 and l + 1 < NL:
            assert not torch.equal(recs[l + 1].x, r.hseq)      # (the mask was applied between the layers)
