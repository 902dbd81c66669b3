"""RNNEncoder (stack of bidirectional LSTMs) -- module API of asr/modeling/encoders/rnn.py:14-81 on the HIP engine.

    encoder(xs, xlens) -> (eouts [B, max elens, enc_hidden_size], elens [B] int64, None)

`rnns` holds one nn.LSTM(bidirectional=True, batch_first=True) per layer as a parameter container (state_dict keys
encoder.rnns.{l}.{weight,bias}_{ih,hh}_l0[_reverse]); the compute is engine/rnn_encoder.py over csrc/bilstm.hip.
"""
import torch.nn as nn

from ..blocks import Conv2dEncoder
from ..functions import rnn_encoder_apply


class RNNEncoder(nn.Module):
    def __init__(self, params):
        super().__init__()
        self.params = params
        self.input_layer = params.input_layer
        self.enc_num_layers = params.enc_num_layers
        if self.input_layer not in ("conv2d", "none"):
            raise NotImplementedError(f"emoasr_amd: input_layer={self.input_layer!r} for the RNN encoder")
        # (a config without the field is not in sum mode either)
        self.enc_hidden_sum_fwd_bwd = bool(getattr(params, "enc_hidden_sum_fwd_bwd", False))
        if not self.enc_hidden_sum_fwd_bwd:
            # the reference keeps hidden_size = enc_hidden_size here (the halved value is only logged, rnn.py:33-39), so its output is
            # 2 * enc_hidden_size wide while every decoder's input layer takes enc_hidden_size: its forward fails on a shape mismatch
            raise NotImplementedError("emoasr_amd: enc_hidden_sum_fwd_bwd=False is broken in the reference (the concatenated "
                                      "output is 2 * enc_hidden_size wide, the decoders take enc_hidden_size); use True")
        input_size = params.feat_dim * params.num_framestacks
        if self.input_layer == "conv2d":
            self.conv = Conv2dEncoder(input_size, params.enc_hidden_size)
            input_size = params.enc_hidden_size
        self.rnns = nn.ModuleList()
        for _ in range(self.enc_num_layers):
            self.rnns.append(nn.LSTM(input_size=input_size, hidden_size=params.enc_hidden_size, num_layers=1, batch_first=True,
                                     bidirectional=True))
            input_size = params.enc_hidden_size
        self._owner = None  # set by ASR so encoder and decoder share one engine / arena

    def forward(self, xs, xlens):
        return rnn_encoder_apply(self, xs, xlens)  # (eouts, elens, None)
