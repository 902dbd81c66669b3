"""Batched LAS beam search against today's single search looped over the same utterances, and the grouped
attention step against ops.las_attend_fwd on replicated rows.

    python tools/las_beam_bench.py [--pairs 5] [--batches 1,16,64] [--widths 4,10]

Prints one JSON line.  Size: tools/las_bench.py's SIZE in bf16, ragged T 200..400 encoder frames, <eos> suppressed so that every
search runs all max_decode_ylen = 60 steps.
  search["B{B}_W{W}"]   ms per utterance of LASDecoder.decode on B utterances: `batch` (las_beam_search_batch: one call, the
                        searches in lockstep) and `loop` (the single search, one call per utterance), host time from the call to
                        the result with the device synchronised, as alternating pairs in ONE process: median and min-max over
                        --pairs, every pair's ratio loop / batch, and the batched search's device time per step;
  attend["rows{S W}"]   us of ONE attention step for S searches of W rows: emoasr_las_attend_group on the stacked memories
                        against emoasr_las_attend_fwd with the memory replicated and padded per row, device time per launch by
                        graph replay (tools/_timing.py), alternating, median and min-max over --pairs.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _timing import graph_time  # noqa: E402
from las_bench import CFG, SIZE, U  # noqa: E402

T_MIN, T_MAX = 200, 400


def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--widths", default="4,10")
    ap.add_argument("--attend-rows", default="1x4,16x4,64x10", help="S x W of the attention-step timings")
    a = ap.parse_args()
    from emoasr_amd import ops
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.functions import _engine_of
    dev, dt = torch.device("cuda"), torch.bfloat16
    torch.manual_seed(0)
    model = ASR(SimpleNamespace(**CFG), compute_dtype=dt).to(dev).eval()
    with torch.no_grad():
        model.decoder.output.bias[CFG["eos_id"]] = -1e4    # <eos> never wins: all U steps run
    dec = model.decoder
    eng = _engine_of(dec)
    g = torch.Generator().manual_seed(1)
    D, A = SIZE["enc_hidden_size"], SIZE["attn_dim"]
    res = {"size": dict(SIZE, T=[T_MIN, T_MAX], U=U), "dtype": "bf16", "pairs": a.pairs, "search": {}, "attend": {}}

    for B in [int(x) for x in a.batches.split(",")]:
        elens = torch.randint(T_MIN, T_MAX + 1, (B,), generator=g)
        elens[0] = T_MAX
        eouts = torch.randn(B, T_MAX, D, generator=g).to(dev, dt)
        el = elens.tolist()
        for W in [int(x) for x in a.widths.split(",")]:
            def batch():
                dec.las_beam_impl = "batch"
                hyps, _, _, _ = dec.decode(eouts, el, None, W, 0.0)
                dec.las_beam_impl = "single"
                assert hyps in ([], [[]] * B)

            def loop():
                for b in range(B):
                    hyps, _, _, _ = dec.decode(eouts[b:b + 1, :el[b]], [el[b]], None, W, 0.0)
                    assert hyps == []

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / B

            batch(); loop()      # warm-up: buffers, the captured steps
            tb, tl, dev_step = [], [], []
            for _ in range(a.pairs):
                eng._las_beam_stats = {"steps": 0, "loop_s": 0.0, "utts": 0, "calls": 0}
                tb.append(timed(batch))
                st = eng._las_beam_stats
                dev_step.append(1e3 * st["loop_s"] / max(st["steps"], 1))
                tl.append(timed(loop))
            res["search"][f"B{B}_W{W}"] = dict(batch_ms_per_utt=stats(tb), loop_ms_per_utt=stats(tl),
                                               loop_over_batch=[round(y / x, 3) for x, y in zip(tb, tl)],
                                               batch_device_ms_per_step=stats(dev_step))

    # ---- one attention step
    sc = dec.score
    Wt = ops.LasWeights(sc.conv.weight.detach().float().contiguous(), sc.w_conv.weight.detach().float().contiguous(),
                        sc.w_conv.bias.detach().float().contiguous(), sc.w_score.weight.detach().float().contiguous())
    for spec in a.attend_rows.split(","):
        S, W = (int(x) for x in spec.split("x"))
        nb = S * W
        Ts = torch.randint(T_MIN, T_MAX + 1, (S,), generator=g).tolist()
        Ts[0] = T_MAX
        moff, offs = ops.las_group_offsets(Ts, dev)
        pk = torch.randn(offs[-1], A, generator=g).to(dev, dt)
        eo = torch.randn(offs[-1], D, generator=g).to(dev, dt)
        pq = torch.randn(nb, A, generator=g).to(dev, dt)
        aw_src = torch.zeros(nb, T_MAX, device=dev)
        for s in range(S):
            aw_src[s * W:(s + 1) * W, :Ts[s]] = torch.softmax(torch.randn(W, Ts[s], generator=g), dim=1).to(dev)
        parent = torch.cat([s * W + torch.randperm(W, generator=g) for s in range(S)]).to(torch.int32).to(dev)
        state = torch.tensor([[1, W, 0, 0]] * S, dtype=torch.int32, device=dev)
        aw_dst, scores = torch.zeros(nb, T_MAX, device=dev), torch.zeros(nb, T_MAX, device=dev)
        ctx = torch.zeros(nb, D, device=dev, dtype=dt)
        rep_pk, rep_eo = torch.zeros(nb, T_MAX, A, device=dev, dtype=dt), torch.zeros(nb, T_MAX, D, device=dev, dtype=dt)
        for s in range(S):
            rep_pk[s * W:(s + 1) * W, :Ts[s]] = pk[offs[s]:offs[s + 1]]
            rep_eo[s * W:(s + 1) * W, :Ts[s]] = eo[offs[s]:offs[s + 1]]
        awp = aw_src.index_select(0, parent.long())
        elr = torch.tensor([Ts[s] for s in range(S) for _ in range(W)], dtype=torch.int32, device=dev)
        aw2, ctx2, lse2, sc2 = torch.zeros(nb, T_MAX, device=dev), torch.zeros_like(ctx), torch.zeros(nb, device=dev), torch.zeros(nb, T_MAX, device=dev)

        def grouped():
            with ops.stream_scope(False):
                ops.las_attend_group(Wt, pk, eo, moff, pq, aw_src, parent, state, W, aw_dst, ctx, scores)

        def replicated():
            with ops.stream_scope(False):
                ops.las_attend_fwd(Wt, rep_pk, pq, awp, rep_eo, elr, aw=aw2, ctx=ctx2, lse=lse2, scores=sc2)

        tg, tr = [], []
        for _ in range(a.pairs):
            tg.append(graph_time(grouped))
            tr.append(graph_time(replicated))
        res["attend"][f"rows{nb}"] = dict(S=S, W=W, grouped_us=stats(tg), replicated_us=stats(tr),
                                          replicated_over_grouped=[round(y / x, 3) for x, y in zip(tg, tr)])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
