"""LAS decoder (decoder_type "las") timings: the teacher-forced decoder per position, the attention step against the same step
composed from torch ops, and beam-4 decoding per output step.

    python tools/las_bench.py [--steps 10] [--warmup 3] [--pairs 5] [--dtype bf16|f32]

Prints one JSON line.  Size (stated in the output): enc_hidden 256, dec_hidden 512, attn_dim 512, embedding 512, intermediate 512,
2 LSTM layers, V = 10 000, B = 32 utterances of T = 400 encoder frames (ragged lengths 200..400), U = 60 decoder positions.
  decoder_fwd_ms_per_pos / decoder_bwd_ms_per_pos   LASDecoder.forward (attention loss + auxiliary CTC) and loss.backward() on given
                       encoder outputs, device time by events, divided by U; median and min-max over --steps runs;
  attend_*_us          ONE attention step for all rows, forward + backward (ops.las_attend_fwd + ops.las_attend_bwd: 3 launches)
                       against the step composed from torch ops with autograd on the same tensors (conv1d, matmul, tanh, masked
                       soft-max, bmm), as alternating legs in ONE process: medians, min-max and every pair's ratio;
  beam4_ms_per_step    LASDecoder.decode(beam_width=4) of one utterance with <eos> suppressed, so that the search runs all
                       max_decode_ylen = 60 steps: host time from the call to the result, divided by 60.
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = dict(enc_hidden_size=256, dec_hidden_size=512, attn_dim=512, embedding_size=512, dec_intermediate_size=512, dec_num_layers=2,
            vocab_size=10000)
B, T, U = 32, 400, 60
CFG = dict(SIZE, input_layer="conv2d", feat_dim=80, num_framestacks=1, encoder_type="transformer", decoder_type="las",
           enc_num_attention_heads=4, enc_num_layers=1, enc_intermediate_size=256, dropout_enc_rate=0.0, dropout_attn_rate=0.0,
           dropout_dec_rate=0.0, blank_id=0, eos_id=2, kd_weight=0, lsm_prob=0.1, loss_normalize_length=False,
           loss_normalize_batch=True, mtl_ctc_weight=0.3, max_decode_ylen=U)


def events(fn, n, warmup):
    out = []
    for i in range(n + warmup):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    a = ap.parse_args()
    from emoasr_amd import ops
    from emoasr_amd.modeling.asr import ASR
    dev = torch.device("cuda")
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    torch.manual_seed(0)
    model = ASR(SimpleNamespace(**CFG), compute_dtype=dt).to(dev).train()
    g = torch.Generator().manual_seed(1)
    elens = torch.randint(T // 2, T + 1, (B,), generator=g)
    elens[0] = T
    ylens = torch.randint(U // 2, U, (B,), generator=g)
    ylens[0] = U - 1
    ys = torch.randint(3, CFG["vocab_size"], (B, U - 1), generator=g)
    eos = torch.full((B, 1), 2)
    ys_in, ys_out = torch.cat([eos, ys], 1), torch.cat([ys, eos], 1)
    eouts = torch.randn(B, T, SIZE["enc_hidden_size"], generator=g).to(dev, dt)
    res = {"size": dict(SIZE, B=B, T=T, U=U), "dtype": a.dtype}

    # ---- the decoder per position
    box = {}

    def fwd():
        e = eouts.clone().requires_grad_(True)
        box["loss"], _, _ = model.decoder(e, elens, None, ys, ylens, ys_in, ys_out)

    def fwd_bwd_only():
        box["loss"].backward()

    tf, tb = [], []
    for i in range(a.steps + a.warmup):
        model.zero_grad()
        f = events(fwd, 1, 0)[0]
        b = events(fwd_bwd_only, 1, 0)[0]
        if i >= a.warmup:
            tf.append(f / U)
            tb.append(b / U)
    res["decoder_fwd_ms_per_pos"], res["decoder_bwd_ms_per_pos"] = stats(tf), stats(tb)

    # ---- one attention step: the kernels against torch ops on the same tensors
    A, D = SIZE["attn_dim"], SIZE["enc_hidden_size"]
    sc = model.decoder.score
    filt, wc, bc, ws = (sc.conv.weight.detach().float().contiguous(), sc.w_conv.weight.detach().float().contiguous(),
                        sc.w_conv.bias.detach().float().contiguous(), sc.w_score.weight.detach().float().contiguous())
    W = ops.LasWeights(filt, wc, bc, ws)
    pk = torch.randn(B, T, A, generator=g).to(dev, dt)
    pq = torch.randn(B, A, generator=g).to(dev, dt)
    pad = torch.arange(T)[None, :] >= elens[:, None]
    awp = torch.softmax(torch.randn(B, T, generator=g).masked_fill(pad, -1e30), dim=1).to(dev)
    dctx = torch.randn(B, D, generator=g).to(dev, dt)
    daw = torch.randn(B, T, generator=g).to(dev)
    el = elens.to(dev, torch.int32)
    pad = pad.to(dev)
    z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
    bufs = dict(dpq=z(B, A), daw_prev=z(B, T), dpk=z(B, T, A), deouts=z(B, T, D), dw_score=z(1, A), dw_conv=z(A, 10), db_conv=z(A),
                dfilt=z(10, 1, 201))

    def fused():
        with ops.stream_scope(False):
            aw, ctx, lse = ops.las_attend_fwd(W, pk, pq, awp, eouts, el, 0.0, 0, 0)
            ops.las_attend_bwd(W, pk, pq, awp, eouts, el, 0.0, 0, 0, aw, ctx, lse, dctx, daw, **bufs)

    leaves = [t.detach().clone().requires_grad_(True) for t in (pk, pq, awp, eouts, filt, wc, bc, ws)]

    def composed():
        lpk, lpq, lawp, leo, lf, lwc, lbc, lws = leaves
        for t in leaves:
            t.grad = None
        feat = torch.nn.functional.conv1d(lawp[:, None, :], lf, padding=100).transpose(1, 2)
        e = torch.tanh(lpk.float() + lpq.float()[:, None, :] + feat @ lwc.t() + lbc) @ lws.view(-1)
        aw = torch.softmax(e.masked_fill(pad, torch.finfo(torch.float32).min), dim=1)
        ctx = torch.bmm(aw[:, None, :].to(leo.dtype), leo)[:, 0]
        ((ctx.float() * dctx.float()).sum() + (aw * daw).sum()).backward()

    tfu, tco, ratios = [], [], []
    for _ in range(a.pairs):
        x = statistics.median(events(fused, a.steps, a.warmup)) * 1e3
        y = statistics.median(events(composed, a.steps, a.warmup)) * 1e3
        tfu.append(x)
        tco.append(y)
        ratios.append(round(y / x, 3))
    res["attend_fused_us"], res["attend_composed_us"], res["attend_composed_over_fused"] = stats(tfu), stats(tco), ratios

    # ---- beam-4 decoding, all max_decode_ylen steps
    model.eval()
    with torch.no_grad():
        model.decoder.output.bias[CFG["eos_id"]] = -1e4
    one = eouts[0:1]
    tbm = []
    for i in range(a.pairs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hyps, _, _, _ = model.decoder.decode(one, torch.tensor([T]), None, 4, 0.0)
        torch.cuda.synchronize()
        if i:
            tbm.append((time.perf_counter() - t0) * 1e3 / U)
        assert hyps == []
    res["beam4_ms_per_step"] = stats(tbm)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
