"""CPU checks of the RNN encoder (encoder_type "rnn"): the module API builds, its state_dict is the reference's, and the fixtures of
tests/golden/make_golden_rnn.py agree with a plain-torch restatement of asr/modeling/encoders/rnn.py (nn.LSTM over packed
sequences) -- which pins the fixtures without a GPU."""
from types import SimpleNamespace

import pytest
import torch

from tests.rnn_util import RNN_FIXTURES, load_rnn_golden, rnn_encoder_cpu


def _asr(cfg):
    from emoasr_amd.modeling.asr import ASR
    return ASR(cfg, compute_dtype=torch.float32)


@pytest.mark.parametrize("name", RNN_FIXTURES)
def test_state_dict_matches_the_reference(name):
    cfg, sd, _ = load_rnn_golden(name)
    model = _asr(cfg)
    mine = model.state_dict()
    assert list(mine) == list(sd)
    for k, v in sd.items():
        assert tuple(mine[k].shape) == tuple(v.shape), k
    model.load_state_dict(sd, strict=True)
    for l in range(cfg.enc_num_layers):
        for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            for sfx in ("", "_reverse"):
                assert f"encoder.rnns.{l}.{kind}_l0{sfx}" in mine
    assert any(k.startswith("encoder.conv.") for k in mine) == (cfg.input_layer == "conv2d")


@pytest.mark.parametrize("name", RNN_FIXTURES)
def test_fixtures_agree_with_packed_nn_lstm(name):
    cfg, sd, g = load_rnn_golden(name)
    with torch.no_grad():
        eouts, elens = rnn_encoder_cpu(cfg, sd, g["xs"], g["xlens"])
    assert torch.equal(elens, g["eval/elens"])
    assert eouts.shape == g["eval/eouts"].shape and eouts.shape[1] == int(elens.max())
    assert (eouts - g["eval/eouts"]).abs().max().item() < 1e-5
    for b, n in enumerate(elens.tolist()):
        assert torch.count_nonzero(g["eval/eouts"][b, n:]) == 0   # pad_packed_sequence's exact zeros
    if "eval/logits" in g:
        logits = eouts @ sd["decoder.output.weight"].t() + sd["decoder.output.bias"]
        assert (logits - g["eval/logits"]).abs().max().item() < 1e-4


def test_the_ragged_lengths_start_every_reverse_direction_elsewhere():
    _, _, g = load_rnn_golden("rnn_ctc_tiny")
    elens = g["eval/elens"].tolist()
    assert len(set(elens)) == len(elens) and min(elens) < max(elens)


def test_concat_mode_is_refused():
    cfg, _, _ = load_rnn_golden("rnn_ctc_tiny")
    bad = SimpleNamespace(**dict(vars(cfg), enc_hidden_sum_fwd_bwd=False))
    with pytest.raises(NotImplementedError, match="enc_hidden_sum_fwd_bwd"):
        _asr(bad)


@pytest.mark.parametrize("decoder_type", ["ctc", "transformer", "rnn_transducer"])
def test_every_decoder_builds_on_the_rnn_encoder(decoder_type):
    cfg, _, _ = load_rnn_golden("rnn_att_tiny")
    extra = dict(embedding_size=64, dec_num_layers=1, joint_hidden_size=128, dropout_emb_rate=0.0)
    model = _asr(SimpleNamespace(**dict(vars(cfg), decoder_type=decoder_type, **extra)))
    assert type(model.encoder).__name__ == "RNNEncoder"
    assert not hasattr(cfg, "enc_num_attention_heads")
