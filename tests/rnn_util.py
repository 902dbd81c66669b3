"""Helpers of the RNN-encoder tests: the fixtures of tests/golden/make_golden_rnn.py (their config travels inside them as JSON)
and a plain-torch CPU restatement of the reference's RNNEncoder (asr/modeling/encoders/rnn.py: Conv2d front-end, then per layer
nn.LSTM(bidirectional=True) over pack_padded_sequence, the directions summed, dropout)."""
import json
from types import SimpleNamespace

import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from tests.util import golden_npz

RNN_FIXTURES = ["rnn_ctc_tiny", "rnn_att_tiny", "rnn_none_tiny"]


def load_rnn_golden(name):
    z = golden_npz(name)
    cfg = json.loads(bytes(z.pop("config")).decode())
    g = {k: torch.from_numpy(v) for k, v in z.items()}
    sd = {k[3:]: v for k, v in g.items() if k.startswith("sd/")}
    return SimpleNamespace(**cfg), sd, g


def lstm_of(sd, prefix, nin, H):
    """an nn.LSTM(bidirectional) holding the state_dict entries under prefix (e.g. "encoder.rnns.0.")"""
    m = nn.LSTM(nin, H, num_layers=1, batch_first=True, bidirectional=True)
    m.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
    return m


def packed_bilstm(m, x, lens):
    """one layer as the reference runs it: packed sequence in, padded output with the two directions summed -> [B, max(lens), H]"""
    packed = pack_padded_sequence(x, torch.as_tensor(lens).cpu(), batch_first=True, enforce_sorted=False)
    y, _ = pad_packed_sequence(m(packed)[0], batch_first=True)
    half = y.shape[-1] // 2
    return y[:, :, :half] + y[:, :, half:]


def rnn_encoder_cpu(cfg, sd, xs, xlens):
    """the reference RNNEncoder's forward (dropout 0) in plain torch -> (eouts, elens)"""
    H = cfg.enc_hidden_size
    xlens = torch.as_tensor(xlens)
    if cfg.input_layer == "conv2d":
        c1 = nn.Conv2d(1, H, 3, 2)
        c2 = nn.Conv2d(H, H, 3, 2)
        c1.weight.data, c1.bias.data = sd["encoder.conv.conv.0.weight"], sd["encoder.conv.conv.0.bias"]
        c2.weight.data, c2.bias.data = sd["encoder.conv.conv.2.weight"], sd["encoder.conv.conv.2.bias"]
        y = torch.relu(c2(torch.relu(c1(xs.unsqueeze(1)))))
        b, c, t, f = y.shape
        x = y.transpose(1, 2).reshape(b, t, c * f) @ sd["encoder.conv.output.weight"].t() + sd["encoder.conv.output.bias"]
        elens = ((xlens - 1) // 2 - 1) // 2
    else:
        x, elens = xs, xlens
    for l in range(cfg.enc_num_layers):
        m = lstm_of(sd, f"encoder.rnns.{l}.", x.shape[-1], H)
        x = packed_bilstm(m, x, elens)
    return x, elens
