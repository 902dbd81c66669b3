"""Device time of the RNN encoder's bidirectional LSTM stack (engine/rnn_encoder.py) per micro-batch, forward and forward + backward,
for the cooperative recurrence (csrc/lstm_coop.hip) and the per-step chain (csrc/bilstm.hip, option lstm_coop = 0), at a
LibriSpeech-like shape (bf16, B 36, T' 350 frames after subsampling, ragged lengths).  Events around each call; median, min and
max over the runs.  The Conv2d
front-end is left out (input_layer "none" with feat_dim = H), so every layer is H -> H; the figures are per layer (both directions
run together in each launch or step).

    python tools/bilstm_bench.py [--B 36] [--T 350] [--H 320 512] [--layers 4] [--iters 7]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench(B, T, H, layers, iters, dev):
    from emoasr_amd.modeling.asr import ASR
    cfg = SimpleNamespace(input_layer="none", feat_dim=H, num_framestacks=1, encoder_type="rnn", decoder_type="ctc",
                          enc_hidden_size=H, enc_num_layers=layers, enc_hidden_sum_fwd_bwd=True, dropout_enc_rate=0.1,
                          vocab_size=64, blank_id=0, eos_id=2, kd_weight=0)
    torch.manual_seed(0)
    model = ASR(cfg, compute_dtype=torch.bfloat16).to(dev).train()
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(int(0.6 * T), T + 1, (B,), generator=g)
    lens[0] = T
    xs = torch.randn(B, T, H, device=dev)

    def fwd():
        with torch.no_grad():
            model.encoder(xs, lens)

    def fwd_bwd():
        eouts, _, _ = model.encoder(xs, lens)
        eouts.float().sum().backward()

    def timed(fn):
        """device time of fn (events around it), median / min / max over `iters` runs after one warm-up"""
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1]

    from emoasr_amd import lib, ops
    rows = []
    for path in ("coop", "chain"):
        with lib.options(lstm_coop=1 if path == "coop" else 0):
            if path == "coop" and not ops.bilstm_seq_supported(xs.to(torch.bfloat16), B, H):
                continue
            f = timed(fwd)
            fb = timed(fwd_bwd)
        r = dict(B=B, T=T, H=H, layers=layers, path=path, iters=iters)
        r["fwd_ms_per_layer"] = [round(v / layers, 3) for v in f]              # median, min, max
        r["fwd_bwd_ms_per_layer"] = [round(v / layers, 3) for v in fb]
        r["bwd_ms_per_layer_median"] = round((fb[0] - f[0]) / layers, 3)
        r["fwd_us_per_step_median"] = round(f[0] / layers * 1e3 / T, 2)
        assert lib.size_query("emoasr_lstm_coop_status") == 0
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=36)
    ap.add_argument("--T", type=int, default=350)
    ap.add_argument("--H", type=int, nargs="+", default=[320, 512])
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--iters", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for H in a.H:
        for r in bench(a.B, a.T, H, a.layers, a.iters, dev):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
