"""The LAS decoder without a GPU: module layout against the reference's state dict, refusals, and tests/las_ref.py -- the float64
restatement that the GPU tests use as their yardstick -- against the reference's goldens (tests/golden/las_tiny*.npz)."""
from types import SimpleNamespace

import pytest
import torch

from tests import las_ref


@pytest.fixture(scope="module")
def fx():
    return las_ref.load_las_golden()


def _decoder(cfg):
    from emoasr_amd.modeling.decoders.las import LASDecoder
    return LASDecoder(SimpleNamespace(**cfg))


def test_state_dict_layout_matches_reference(fx):
    from emoasr_amd.modeling.asr import ASR
    cfg, sd, _ = fx
    alone = _decoder(cfg).state_dict()
    assert {"decoder." + k for k in alone} == set(sd)
    for k, v in alone.items():
        assert tuple(v.shape) == tuple(sd["decoder." + k].shape), k
    assert tuple(sd["decoder.score.conv.weight"].shape) == (10, 1, 201) and "decoder.score.conv.bias" not in sd
    assert "decoder.rnns.0.weight_ih" in sd and tuple(sd["decoder.rnns.0.weight_ih"].shape) == (4 * 96, 64 + 128)
    model = ASR(SimpleNamespace(**las_ref.las_asr_config(cfg)))
    mine = {k: v for k, v in model.state_dict().items() if k.startswith("decoder.")}
    assert set(mine) == set(sd)
    assert all(tuple(mine[k].shape) == tuple(sd[k].shape) for k in sd)
    assert model.decoder.ctc._owner[0] is model and model.decoder._owner[0] is model


def test_reference_checkpoint_loads(fx):
    from emoasr_amd.modeling.asr import ASR
    cfg, sd, _ = fx
    dec = _decoder(cfg)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in sd.items()})   # strict
    assert torch.equal(dec.rnns[1].weight_hh, sd["decoder.rnns.1.weight_hh"])
    model = ASR(SimpleNamespace(**las_ref.las_asr_config(cfg)))
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.startswith("encoder.") for k in res.missing_keys)
    assert model.decoder.score.dropout_attn_rate == 0.1   # AttentionLoc's constructor default: no config field reaches it


def test_missing_fields_raise_by_name(fx):
    from emoasr_amd.modeling.decoders.las import LAS_FIELDS
    cfg = fx[0]
    for f in LAS_FIELDS:
        with pytest.raises(AttributeError, match=f):
            _decoder({k: v for k, v in cfg.items() if k != f})


@pytest.mark.parametrize("field", ["embedding_size", "enc_hidden_size", "dec_hidden_size", "attn_dim", "dec_intermediate_size"])
def test_unsupported_sizes_raise(fx, field):
    with pytest.raises(NotImplementedError, match=field):
        _decoder(dict(fx[0], **{field: fx[0][field] + 4}))
    if field == "attn_dim":
        with pytest.raises(NotImplementedError, match="attn_dim"):
            _decoder(dict(fx[0], attn_dim=520))


def test_other_decoders_stay_refused(fx):
    from emoasr_amd.modeling.asr import ASR
    with pytest.raises(NotImplementedError):
        ASR(SimpleNamespace(**dict(las_ref.las_asr_config(fx[0]), decoder_type="las2")))


@pytest.mark.parametrize("case", ["a", "b", "kd"])
def test_las_ref_equals_the_goldens(fx, case):
    """losses to 1e-7 (the f32 soft labels' rows sum to 1 only to 1e-7, and the two statements of the distillation loss weigh the
    log-partition by that sum differently; without soft labels they agree to 1e-12), logits on the valid positions and every gradient
    to 1e-5 of the largest (the fixture stores them as f32)"""
    cfg, sd, g = fx
    cfg = SimpleNamespace(**dict(cfg, kd_weight=0.5 if case == "kd" else 0))
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    eouts = g[f"{case}/eouts"].double().requires_grad_(True)
    soft = g["kd/soft"].double() if case == "kd" else None
    out = las_ref.decoder_forward(sd64, cfg, eouts, g[f"{case}/elens"], g[f"{case}/ys"], g[f"{case}/ylens"], g[f"{case}/ys_in"],
                                  g[f"{case}/ys_out"], soft)
    for k in ("loss_total", "loss_att", "loss_ctc") + (("loss_kd",) if case == "kd" else ()):
        assert abs(out[k].item() - g[f"{case}/{k}"].item()) <= (1e-7 if case == "kd" else 1e-12) * abs(g[f"{case}/{k}"].item()), k
    ref = g[f"{case}/logits"].double()
    ok = las_ref.valid_positions(g[f"{case}/ylens"], ref.shape[1])
    assert ((out["logits"].detach() - ref)[ok].abs().max() / ref.abs().max()).item() <= 1e-6
    out["loss_total"].backward()
    grads = {k[len(case) + 6:]: v for k, v in g.items() if k.startswith(case + "/grad/")}
    assert set(grads) == set(sd)
    gmax = max(v.abs().max().item() for v in grads.values())
    for k, v in grads.items():
        got = sd64[k].grad if sd64[k].grad is not None else torch.zeros_like(sd64[k])
        assert ((got - v.double()).abs().max() / gmax).item() <= 1e-5, k
    assert ((eouts.grad - g[f"{case}/deouts"].double()).abs().max() / g[f"{case}/deouts"].abs().max()).item() <= 1e-5
    # shift invariance of the soft-max: the score bias receives nothing
    assert grads["decoder.score.w_score.bias"].abs().max().item() <= 1e-9 * gmax


def test_rows_are_independent_past_their_lengths(fx):
    """garbage labels past ylens + 1 of a row change neither the loss nor a gradient"""
    cfg, sd, g = fx
    cfg = SimpleNamespace(**cfg)
    res = []
    for garble in (False, True):
        ys_in, ys_out = g["a/ys_in"].clone(), g["a/ys_out"].clone()
        if garble:
            for b, n in enumerate(g["a/ylens"].tolist()):
                ys_in[b, n + 1:] = 7
                ys_out[b, n + 1:] = 9
        sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        out = las_ref.decoder_forward(sd64, cfg, g["a/eouts"].double(), g["a/elens"], g["a/ys"], g["a/ylens"], ys_in, ys_out)
        out["loss_total"].backward()
        res.append((out["loss_total"].item(), sd64["decoder.score.conv.weight"].grad.clone()))
    assert abs(res[0][0] - res[1][0]) <= 1e-12 * abs(res[0][0]) and torch.allclose(res[0][1], res[1][1], rtol=0, atol=1e-12)


def test_f32_kernel_floor_constant():
    """tests/test_las_gpu.py holds the f32 kernels to 4 x the error the restatement itself makes when it runs in f32 torch on the
    CPU, largest over the seeded cases and over every output and gradient"""
    from tests.test_las_gpu import KERNEL_F32_FLOOR
    worst = 0.0
    for T in las_ref.KERNEL_T:
        for ragged in (False, True):
            errs = las_ref.step_errors(las_ref.step_in_dtype(T, ragged, torch.float32), las_ref.step_in_dtype(T, ragged, torch.float64))
            worst = max(worst, max(errs.values()))
    assert abs(worst - KERNEL_F32_FLOOR) <= 0.25 * KERNEL_F32_FLOOR, worst


def test_bf16_logit_error_constant(fx):
    """tests/test_las_gpu.py holds the bf16 logits to 4 x the error of this simulation: the restatement with matrices and stored
    activations rounded to bf16 against itself in f64, largest |difference| over the valid positions, of the logits' range"""
    from tests.test_las_gpu import LAS_LOGITS_BF16_SIM
    cfg, sd, g = fx
    cfg = SimpleNamespace(**cfg)
    rnd = lambda x: x.to(torch.bfloat16).to(x.dtype)
    sd64 = {k: v.double() for k, v in sd.items()}
    for case in ("a", "b"):
        args = (sd64, cfg, g[f"{case}/eouts"].double(), g[f"{case}/elens"], g[f"{case}/ys"], g[f"{case}/ylens"], g[f"{case}/ys_in"],
                g[f"{case}/ys_out"])
        a, b = las_ref.decoder_forward(*args)["logits"], las_ref.decoder_forward(*args, rnd=rnd)["logits"]
        ok = las_ref.valid_positions(g[f"{case}/ylens"], a.shape[1])
        sim = ((a - b)[ok].abs().max() / a.abs().max()).item()
        assert abs(sim - LAS_LOGITS_BF16_SIM[case]) <= 0.02 * LAS_LOGITS_BF16_SIM[case], (case, sim)
