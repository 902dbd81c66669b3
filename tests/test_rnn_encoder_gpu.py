"""The RNN encoder (encoder_type "rnn": bidirectional LSTMs over packed sequences, csrc/bilstm.hip + engine/rnn_encoder.py) on the GPU.

Bars: f32 / f32x3 as tests/test_model_gpu.py (1e-3 on loss / logits, greedy ids bit-exact, gradients to rtol 1e-3; the layer alone
to 1e-5); bf16 loss 2e-2, outputs 6e-2 of their range, gradients by cosine."""
from types import SimpleNamespace

import pytest
import torch

from tests.rnn_util import load_rnn_golden, lstm_of, packed_bilstm
from tests.util import split_ragged

pytestmark = pytest.mark.gpu

F32X3 = "f32x3"
MODES = [torch.float32, F32X3, torch.bfloat16]
MODE_IDS = ["f32", "f32x3", "bf16"]


def _rel(a, b):
    return ((a.float().cpu() - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _cos(a, b):
    a, b = a.float().cpu().flatten(), b.float().flatten()
    return (torch.dot(a, b) / (a.norm() * b.norm() + 1e-30)).item()


def _layer_model(nin, H, layers, dtype, dev, seed=0):
    """input_layer "none": the encoder is the LSTM stack alone (xs -> layer 0)"""
    from emoasr_amd.modeling.asr import ASR
    cfg = SimpleNamespace(input_layer="none", feat_dim=nin, num_framestacks=1, encoder_type="rnn", decoder_type="ctc",
                          enc_hidden_size=H, enc_num_layers=layers, enc_hidden_sum_fwd_bwd=True, dropout_enc_rate=0.0,
                          vocab_size=16, blank_id=0, eos_id=2, kd_weight=0)
    torch.manual_seed(seed)
    model = ASR(cfg, compute_dtype=dtype)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    return model.to(dev), sd, cfg


def _ragged(B, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    lens[min(1, B - 1)] = 1 if B > 1 else T
    return lens


def _cpu_stack(sd, xs, lens, H, layers):
    x = xs
    for l in range(layers):
        x = packed_bilstm(lstm_of(sd, f"encoder.rnns.{l}.", x.shape[-1], H), x, lens)
    return x


# ---- (a) op level, forward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", [(3, 64), (70, 128), (200, 64), (70, 512), (3, 512)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_layer_forward_against_packed_nn_lstm(dev, B, H, dtype):
    T, nin = 23, 40
    model, sd, _ = _layer_model(nin, H, 1, dtype, dev)
    lens = _ragged(B, T, seed=B + H)
    xs = torch.randn(B, T, nin)
    for b, n in enumerate(lens.tolist()):
        xs[b, n:] = 0
    model.eval()
    with torch.no_grad():
        eouts, elens, _ = model.encoder(xs.to(dev), lens)
        want = _cpu_stack(sd, xs, lens, H, 1)
    assert eouts.shape == want.shape
    for b, n in enumerate(lens.tolist()):
        assert torch.count_nonzero(eouts[b, n:]) == 0
    if dtype == torch.float32:
        assert (eouts.cpu() - want).abs().max().item() < 1e-5
    else:
        assert _rel(eouts, want) < 3e-2, _rel(eouts, want)


def _coop_ok(dev, B, H):
    from emoasr_amd import ops
    return ops.bilstm_seq_supported(torch.empty(0, device=dev, dtype=torch.bfloat16), B, H)


def _run_layer(model, xs, lens, R, dev):
    model.zero_grad(set_to_none=False)
    eouts, _, _ = model.encoder(xs.to(dev), lens)
    (eouts.float() * R.to(dev)).sum().backward()
    return eouts.detach().float().cpu(), {n: p.grad.detach().clone().cpu() for n, p in model.named_parameters()
                                          if n.startswith("encoder.")}


@pytest.mark.parametrize("B,H", [(3, 64), (70, 128), (200, 64), (70, 512), (3, 512)])
def test_cooperative_matches_the_chain(dev, B, H):
    """bf16: the one-launch bidirectional recurrence (csrc/lstm_coop.hip) against the per-step chain (option lstm_coop = 0), forward
    and backward, lengths 1 and T' included; the two agree to bf16 rounding (different k order, the chain's products rounded)"""
    from emoasr_amd import lib
    assert _coop_ok(dev, B, H)
    T, nin = 23, 40
    model, sd, _ = _layer_model(nin, H, 2, torch.bfloat16, dev, seed=H)
    model.train()
    lens = _ragged(B, T, seed=B * H)
    xs, R = torch.randn(B, T, nin), torch.randn(B, T, H)
    y_coop, g_coop = _run_layer(model, xs, lens, R, dev)
    assert lib.size_query("emoasr_lstm_coop_status") == 0
    with lib.options(lstm_coop=0):
        assert not _coop_ok(dev, B, H)
        y_chain, g_chain = _run_layer(model, xs, lens, R, dev)
    for b, n in enumerate(lens.tolist()):
        assert torch.count_nonzero(y_coop[b, n:]) == 0 and torch.count_nonzero(y_chain[b, n:]) == 0
    assert _rel(y_coop, y_chain) < 2e-2, _rel(y_coop, y_chain)
    assert _rel(y_coop, _cpu_stack(sd, xs, lens, H, 2)) < 3e-2
    for n in g_coop:
        assert _cos(g_coop[n], g_chain[n]) > 0.999, (n, _cos(g_coop[n], g_chain[n]))


# ---- (b) op level, backward: lengths where a wrong W_hh pairing across an utterance boundary (or a t + 1 shift) shows -------------
@pytest.mark.parametrize("dtype", [torch.float32, F32X3], ids=["f32", "f32x3"])
def test_layer_backward_against_cpu_autograd(dev, dtype):
    B, T, nin, H = 5, 17, 24, 64
    model, sd, _ = _layer_model(nin, H, 2, dtype, dev, seed=3)
    lens = torch.tensor([17, 1, 9, 16, 2])
    xs = torch.randn(B, T, nin)
    R = torch.randn(B, T, H)
    model.train()
    eouts, _, _ = model.encoder(xs.to(dev), lens)
    (eouts.float() * R.to(dev)).sum().backward()
    ref = {}
    x = xs
    for l in range(2):
        m = lstm_of(sd, f"encoder.rnns.{l}.", x.shape[-1], H)
        ref.update((f"encoder.rnns.{l}.{n}", p) for n, p in m.named_parameters())
        x = packed_bilstm(m, x, lens)
    (x * R).sum().backward()
    got = dict(model.named_parameters())
    assert set(ref) == {k for k in got if k.startswith("encoder.")}
    for k, v in ref.items():
        gp = got[k].grad.cpu()
        err = (gp - v.grad).abs().max().item() / (v.grad.abs().max().item() + 1e-12)
        assert err < 1e-3, (k, err)


# ---- (c) model level against the reference's fixtures ----------------------------------------------------------------------------
def _golden_model(name, dtype, dev):
    from emoasr_amd.modeling.asr import ASR
    cfg, sd, g = load_rnn_golden(name)
    model = ASR(cfg, compute_dtype=dtype)
    model.load_state_dict(sd)
    return model.to(dev), cfg, sd, g


@pytest.mark.parametrize("name", ["rnn_ctc_tiny", "rnn_none_tiny", "rnn_att_tiny"])
@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_model_against_the_fixtures(dev, name, dtype):
    model, cfg, sd, g = _golden_model(name, dtype, dev)
    f32 = dtype != torch.bfloat16
    xs = g["xs"].to(dev)
    model.train()
    loss, loss_dict = model(xs, g["xlens"], g["ys"], g["ylens"], g["ys_in"], g["ys_out"])
    loss.backward()
    ltol = 1e-3 if f32 else 2e-2
    assert abs(loss.item() - g["train/loss"].item()) < ltol * abs(g["train/loss"].item()), (loss.item(), g["train/loss"].item())
    for k in ("loss_ctc", "loss_att"):
        if "train/" + k in g:
            want = g["train/" + k].item()
            got = float(loss_dict[k].detach())
            assert abs(got - want) < ltol * abs(want), (k, got, want)
    # (a gradient that is zero in exact arithmetic -- the key projection's bias under softmax -- is held to the largest one's scale)
    gmax = max(g["grad/" + n].abs().max().item() for n, _ in model.named_parameters())
    for n, p in model.named_parameters():
        want = g["grad/" + n]
        if f32:
            err = (p.grad.cpu() - want).abs().max().item() / max(want.abs().max().item(), 1e-4 * gmax)
            assert err < 1e-3, (n, err)
        else:
            assert want.abs().max().item() < 1e-4 * gmax or _cos(p.grad, want) > 0.98, (n, _cos(p.grad, want))
    model.eval()
    with torch.no_grad():
        eouts, elens, inter = model.encoder(xs, g["xlens"])
        assert inter is None and torch.equal(elens.cpu(), g["eval/elens"])
        tol = 1e-3 if f32 else 6e-2
        assert _rel(eouts, g["eval/eouts"]) < tol
        if "eval/logits" in g:
            assert _rel(model.decoder(eouts, elens), g["eval/logits"]) < tol
        else:
            assert _rel(model.decoder(eouts, elens, None, g["ys"], g["ylens"], g["ys_in"], None), g["eval/att_logits"]) < tol
    if "eval/hyps" in g:
        hyps, _, _, _ = model.decode(xs, g["xlens"], beam_width=1)
        want = split_ragged(g["eval/hyps"], g["eval/hyp_lens"])
        if f32:
            assert hyps == want
        else:
            assert sum(len(h) for h in hyps) > 0


# ---- (d) padding invariance ------------------------------------------------------------------------------------------------------
def test_padding_changes_nothing(dev):
    model, cfg, sd, g = _golden_model("rnn_ctc_tiny", torch.bfloat16, dev)
    xs, xlens = g["xs"], g["xlens"]
    noisy = torch.cat([xs, torch.zeros(xs.shape[0], 37, xs.shape[2])], 1)
    gen = torch.Generator().manual_seed(5)
    for b, n in enumerate(xlens.tolist()):
        noisy[b, n:] = torch.randn(noisy.shape[1] - n, xs.shape[2], generator=gen)
    model.train()
    outs, grads = [], []
    for x in (xs, noisy):
        model.zero_grad(set_to_none=False)
        eouts, elens, _ = model.encoder(x.to(dev), xlens)
        R = torch.randn(eouts.shape, generator=torch.Generator().manual_seed(1)).to(dev)
        (eouts.float() * R).sum().backward()
        outs.append(eouts.detach().clone())
        grads.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if n.startswith("encoder.")})
    assert outs[0].shape == outs[1].shape
    assert torch.equal(outs[0], outs[1])
    # the gradients: every padded row contributes exact zeros, but the weight / bias gradient products reduce over rows with f32
    # atomics across workgroups, whose order varies from run to run -- held to f32 summation noise rather than bit for bit
    for n in grads[0]:
        err = (grads[0][n] - grads[1][n]).abs().max().item() / grads[0][n].abs().max().item()
        assert err < 1e-5, (n, err)


# ---- (e) changing grid sizes in one process -------------------------------------------------------------------------------------
def test_changing_shapes_in_one_process(dev):
    """cooperative launches whose grid (2 directions x ceil(B / 64) groups x H / 16 workgroups) changes from call to call: the
    host-tracked barrier bases must stay exact, forward and backward"""
    from emoasr_amd import lib
    for B, H in [(3, 64), (130, 128), (1, 32), (200, 256), (64, 512), (3, 64)]:
        assert _coop_ok(dev, B, H), (B, H)
        model, sd, _ = _layer_model(16, H, 1, torch.bfloat16, dev, seed=B)
        lens = _ragged(B, 11, seed=H)
        xs = torch.randn(B, 11, 16)
        model.train()
        eouts, _, _ = model.encoder(xs.to(dev), lens)
        eouts.float().sum().backward()
        want = _cpu_stack(sd, xs, lens, H, 1)
        assert _rel(eouts.detach(), want) < 3e-2, (B, H)
        assert all(torch.isfinite(p.grad).all() for p in model.parameters())
        assert lib.size_query("emoasr_lstm_coop_status") == 0, (B, H)


# ---- (f) training driver, decoding -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rnn_ctc_tiny", "rnn_att_tiny"])
def test_train_step_and_decode(dev, name):
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.optimizers import Adam
    from emoasr_amd.train import train_step
    cfg, sd, g = load_rnn_golden(name)
    params = SimpleNamespace(**dict(vars(cfg), dropout_enc_rate=0.1, accum_grad=1, clip_grad_norm=5.0))
    model = ASR(params, compute_dtype=torch.bfloat16)
    model.load_state_dict(sd)
    optimizer = Adam(model.parameters(), lr=1e-3)
    model.to(dev)
    assert not model.engine().encoder_stacked_ok()
    seen = []
    model.engine().grad_hook = seen.append
    data = {k: g[k] for k in ("xs", "xlens", "ys", "ylens", "ys_in", "ys_out")}
    model.train()
    losses = [train_step(model, optimizer, data, params, dev)["loss_total"] for _ in range(6)]
    assert all(torch.isfinite(torch.tensor(losses))), losses
    assert losses[-1] < losses[0], losses
    lo = min(o for n, o in model.engine().arena.offsets.items() if n.startswith("encoder.rnns.0."))
    assert lo in seen, (lo, seen)
    model.eval()
    if name == "rnn_ctc_tiny":
        hyps, _, _, _ = model.decode(g["xs"].to(dev), g["xlens"], beam_width=1)
        assert len(hyps) == g["xs"].shape[0]
    else:   # (the attention decoder's search takes one utterance at a time)
        b = 0
        n = int(g["xlens"][b])
        hyps, scores, _, _ = model.decode(g["xs"][b:b + 1, :n].to(dev), g["xlens"][b:b + 1], beam_width=4, decode_ctc_weight=0.3)
        assert len(hyps) >= 1 and all(isinstance(t, int) for t in hyps[0])


def test_joint_beam_search_matches_the_reference(dev):
    model, cfg, sd, g = _golden_model("rnn_att_tiny", torch.float32, dev)
    model.eval()
    for b in range(2):
        n = int(g["xlens"][b])
        hyps, scores, _, _ = model.decode(g["xs"][b:b + 1, :n].to(dev), g["xlens"][b:b + 1], beam_width=4, len_weight=0.0,
                                          lm_weight=0.0, decode_ctc_weight=0.3)
        want = split_ragged(g[f"beam/{b}/hyps"], g[f"beam/{b}/lens"])
        assert hyps == want, (b, hyps, want)   # (on these weights the reference's search ends no hypothesis: an empty n-best)


# ---- (g) transducer decoder on the RNN encoder ------------------------------------------------------------------------------------
def test_rnn_transducer_on_the_rnn_encoder(dev):
    from emoasr_amd.modeling.asr import ASR
    cfg, sd, g = load_rnn_golden("rnn_ctc_tiny")
    params = SimpleNamespace(**dict(vars(cfg), decoder_type="rnn_transducer", embedding_size=64, dec_hidden_size=128,
                                    dec_num_layers=1, joint_hidden_size=128, dropout_emb_rate=0.0, mtl_ctc_weight=0.3))
    torch.manual_seed(0)
    model = ASR(params, compute_dtype=torch.bfloat16)
    model.load_state_dict({k: v for k, v in sd.items() if k.startswith("encoder.")}, strict=False)
    model.to(dev).train()
    loss, _ = model(g["xs"].to(dev), g["xlens"], g["ys"], g["ylens"], g["ys_in"], g["ys_out"])
    loss.backward()
    assert torch.isfinite(loss).item()
    for n, p in model.named_parameters():
        if n.startswith("encoder.rnns."):
            assert p.grad.abs().max().item() > 0, n
    model.eval()
    hyps, _, _, _ = model.decode(g["xs"].to(dev), g["xlens"], beam_width=1)
    assert len(hyps) == g["xs"].shape[0]
