"""Golden vectors of the RNN encoder (encoder_type "rnn", asr/modeling/encoders/rnn.py) from the reference at /root/reference.

Runs ONLY in the authoring container (the reference cannot travel); writes data-only fixtures next to this script, each sharded
below tests/util.py SHARD_BYTES.  tests/test_rnn_encoder_cpu.py pins them against a plain torch restatement, and
tests/test_rnn_encoder_gpu.py pins the HIP engine against them.

    python tests/golden/make_golden_rnn.py
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ASR, make_batch, make_params, save_npz  # noqa: E402  (puts the reference on sys.path)

RNN = dict(input_layer="conv2d", feat_dim=40, num_framestacks=1, encoder_type="rnn", decoder_type="ctc", enc_hidden_size=128,
           enc_num_layers=2, enc_hidden_sum_fwd_bwd=True, dropout_enc_rate=0.0, dropout_dec_rate=0.0, dropout_attn_rate=0.0,
           vocab_size=40, blank_id=0, eos_id=2, kd_weight=0, lsm_prob=0.1)
CONFIGS = {
    "rnn_ctc_tiny": RNN,
    "rnn_att_tiny": dict(RNN, decoder_type="transformer", dec_hidden_size=128, dec_num_attention_heads=2, dec_num_layers=2,
                         dec_intermediate_size=256, mtl_ctc_weight=0.3, loss_normalize_length=False, loss_normalize_batch=True,
                         max_decode_ylen=20),
    "rnn_none_tiny": dict(RNN, input_layer="none", enc_num_layers=1),
}
BEAM = dict(beam_width=4, len_weight=0.0, lm_weight=0.0, decode_ctc_weight=0.3)


def run(name, cfg):
    torch.manual_seed(0)
    model = ASR(make_params(cfg), phase="train")
    with torch.no_grad():
        model.decoder.output.weight.mul_(3.0)   # a wider spread: greedy decoding is not dominated by ties
        if cfg["decoder_type"] == "transformer":
            model.decoder.output.bias[cfg["eos_id"]] += 6.0   # random-init decoders never emit <eos> otherwise
    xs, xlens, ys, ylens, ys_in, ys_out = make_batch(1, cfg["feat_dim"], cfg["vocab_size"])
    out = {"config": np.frombuffer(json.dumps(cfg, sort_keys=True).encode(), dtype=np.uint8)}
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    for k, v in sd0.items():
        out["sd/" + k] = v.numpy()
    out.update(xs=xs.numpy(), xlens=xlens.numpy(), ys=ys.numpy(), ylens=ylens.numpy(), ys_in=ys_in.numpy(), ys_out=ys_out.numpy())
    model.train()
    loss, loss_dict = model(xs, xlens, ys, ylens, ys_in, ys_out)
    loss.backward()
    out["train/loss"] = loss.detach().numpy()
    for k, v in loss_dict.items():
        if k != "loss_total" and v is not None:
            out["train/" + k] = torch.as_tensor(v).detach().numpy()
    for n, p in model.named_parameters():
        out["grad/" + n] = p.grad.clone().numpy()
    model.load_state_dict(sd0)
    model.eval()
    with torch.no_grad():
        eouts, elens, _ = model.encoder(xs, xlens)
        out["eval/eouts"] = eouts.numpy()
        out["eval/elens"] = elens.numpy()
        if cfg["decoder_type"] == "ctc":
            out["eval/logits"] = model.decoder(eouts, elens).numpy()
            hyps, _, _, _ = model.decode(xs, xlens, beam_width=1)
            out["eval/hyp_lens"] = np.array([len(h) for h in hyps])
            out["eval/hyps"] = np.array(sum(hyps, []), dtype=np.int64)
        else:
            out["eval/att_logits"] = model.decoder(eouts, elens, None, ys, ylens, ys_in, None).numpy()
            for b in range(2):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    hyps, scores, _, _ = model.decode(xs[b:b + 1, : xlens[b]], xlens[b:b + 1], **BEAM)
                out[f"beam/{b}/lens"] = np.array([len(h) for h in hyps])
                out[f"beam/{b}/hyps"] = np.array(sum(hyps, []), dtype=np.int64)
                out[f"beam/{b}/scores"] = np.array(scores, dtype=np.float64)
    save_npz(name, out)
    print(name, "loss", float(loss.detach()), {k: float(v) for k, v in loss_dict.items() if v is not None},
          "params", sum(p.numel() for p in model.parameters()))


if __name__ == "__main__":
    for name in sys.argv[1:] or list(CONFIGS):
        run(name, CONFIGS[name])
