"""RNN-LM shallow fusion in the LAS beam search: the fused device search against the host form and the unfused
device search, the (lm_weight, len_weight) grid in one call against one call per cell, and emoasr_las_attend_cells against
emoasr_las_attend_group on replicated frames.

    python tools/las_fusion_bench.py [--pairs 5] [--batches 1,16,64] [--widths 4,10] [--host-utts 8]

Prints one JSON line.  Protocol of tools/las_beam_bench.py: its model size in bf16 plus a 2-layer RNN LM with E = H = 512 over the
same vocabulary, ragged T 200..400 encoder frames, <eos> suppressed so that every search runs all max_decode_ylen = 60 steps; host
time from the call to the result with the device synchronised; the legs of one figure alternate in ONE process; median, min and max
over --pairs.
  search["B{B}_W{W}"]   ms per utterance of LASDecoder.decode on B utterances: `fused` (las_lm_fusion = "fuse": one batched device
                        search with the LM stepped inside the chain), `unfused` (the same call under "ignore") and `host` (the host
                        form, one call per utterance, over the first min(B, --host-utts) utterances: its searches are independent);
                        every pair's ratios fused / unfused and host / fused.
  grid["B{B}_W{W}"]     s of the default 11 x 6 grid on B utterances: `one_call` (las_fusion_grid_apply: ten fused searches and one
                        unfused per utterance, the len_weights expanded on the host) and `per_cell` = 6 x the timed cell (0, 0) + 60
                        x the mean of the timed cells (0.5, 0) and (1.0, 5), each ONE batched decode call -- three cells are timed,
                        the other 63 are scaled from them.
  attend["U{U}_W{W}"]   us of ONE attention step for U utterances of 11 searches of W rows each: emoasr_las_attend_cells on frames
                        stored once per utterance against emoasr_las_attend_group on frames replicated per search, device time per
                        launch by graph replay (tools/_timing.py).
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _timing import graph_time  # noqa: E402
from las_bench import CFG, SIZE, U as STEPS  # noqa: E402

T_MIN, T_MAX = 200, 400
LM_CFG = dict(lm_type="rnn", vocab_size=SIZE["vocab_size"], embedding_size=512, hidden_size=512, num_layers=2, dropout_rate=0.0,
              tie_weights=False)
PER_UTT = 11          # searches of one utterance in the attention leg: the distinct lm_weights of the default grid


def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def timed(fn, per=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--widths", default="4,10")
    ap.add_argument("--host-utts", type=int, default=8)
    ap.add_argument("--grid-batch", type=int, default=16)
    ap.add_argument("--grid-widths", default="4,10")
    ap.add_argument("--attend", default="16x4,16x10", help="U x W of the attention-step timings")
    a = ap.parse_args()
    from emoasr_amd import ops
    from emoasr_amd.fusion_grid import weight_lists
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.functions import las_fusion_grid_apply, las_rnnlm_why_not
    from emoasr_amd.modeling.lm import LM
    dev, dt = torch.device("cuda"), torch.bfloat16
    torch.manual_seed(0)
    model = ASR(SimpleNamespace(**CFG), compute_dtype=dt).to(dev).eval()
    lm = LM(SimpleNamespace(**LM_CFG), compute_dtype=dt).to(dev).eval()
    with torch.no_grad():
        model.decoder.output.bias[CFG["eos_id"]] = -1e4    # <eos> never wins: all steps run, with or without the LM
    dec = model.decoder
    assert las_rnnlm_why_not(dec, 10, lm) is None
    g = torch.Generator().manual_seed(1)
    D, A = SIZE["enc_hidden_size"], SIZE["attn_dim"]
    res = {"size": dict(SIZE, T=[T_MIN, T_MAX], U=STEPS), "lm": LM_CFG, "dtype": "bf16", "pairs": a.pairs, "host_utts": a.host_utts,
           "search": {}, "grid": {}, "attend": {}}

    def utterances(B):
        elens = torch.randint(T_MIN, T_MAX + 1, (B,), generator=g)
        elens[0] = T_MAX
        return torch.randn(B, T_MAX, D, generator=g).to(dev, dt), elens.tolist()

    def decode(eouts, el, W, mode, lw=0.0, a_lm=0.5):
        dec.las_lm_fusion, dec.las_beam_impl = mode, "batch"
        try:
            hyps, _, _, _ = dec.decode(eouts, el, None, W, lw, lm=lm, lm_weight=a_lm)
        finally:
            dec.las_lm_fusion, dec.las_beam_impl = "ignore", "single"
        assert hyps in ([], [[]] * len(el))

    # ---- the searches
    for B in [int(x) for x in a.batches.split(",")]:
        eouts, el = utterances(B)
        nh = min(B, a.host_utts)
        for W in [int(x) for x in a.widths.split(",")]:
            def host():
                dec.las_lm_fusion = "fuse"
                try:
                    for b in range(nh):
                        hyps, _, _, _ = dec.decode(eouts[b:b + 1, :el[b]], [el[b]], None, W, 0.0, lm=lm, lm_weight=0.5)
                        assert hyps == []
                finally:
                    dec.las_lm_fusion = "ignore"

            fused = lambda: decode(eouts, el, W, "fuse")
            unfused = lambda: decode(eouts, el, W, "ignore")
            fused(); unfused(); host()      # warm-up: buffers, the captured steps
            tf, tu, th = [], [], []
            for _ in range(a.pairs):
                tf.append(timed(fused, B))
                tu.append(timed(unfused, B))
                th.append(timed(host, nh))
            res["search"][f"B{B}_W{W}"] = dict(fused_ms_per_utt=stats(tf), unfused_ms_per_utt=stats(tu), host_ms_per_utt=stats(th),
                                               fused_over_unfused=[round(x / y, 3) for x, y in zip(tf, tu)],
                                               host_over_fused=[round(y / x, 3) for x, y in zip(tf, th)])

    # ---- the grid
    lm_weights, len_weights = weight_lists(0, 1, 0.1, 0, 5, 1)
    assert len(lm_weights) == 11 and len(len_weights) == 6
    B = a.grid_batch
    eouts, el = utterances(B)
    for W in [int(x) for x in a.grid_widths.split(",")]:
        def one_call():
            hyps, _ = las_fusion_grid_apply(dec, eouts, el, W, lm, lm_weights, len_weights)
            assert len(hyps) == B and all(len(h) == 66 and not any(h) for h in hyps)

        cells = {"c0_0": lambda: decode(eouts, el, W, "ignore", 0.0, 0.0), "c05_0": lambda: decode(eouts, el, W, "fuse", 0.0, 0.5),
                 "c1_5": lambda: decode(eouts, el, W, "fuse", 5.0, 1.0)}
        one_call()
        for fn in cells.values():
            fn()
        t1, tc = [], {k: [] for k in cells}
        for _ in range(a.pairs):
            t1.append(timed(one_call) / 1e3)
            for k, fn in cells.items():
                tc[k].append(timed(fn) / 1e3)
        per_cell = [6 * x + 30 * (y + z) for x, y, z in zip(tc["c0_0"], tc["c05_0"], tc["c1_5"])]
        res["grid"][f"B{B}_W{W}"] = dict(one_call_s=stats(t1), per_cell_s=stats(per_cell), timed_cells_s={k: stats(v) for k, v in tc.items()},
                                         per_cell_over_one_call=[round(y / x, 3) for x, y in zip(t1, per_cell)])

    # ---- one attention step
    sc = dec.score
    Wt = ops.LasWeights(sc.conv.weight.detach().float().contiguous(), sc.w_conv.weight.detach().float().contiguous(),
                        sc.w_conv.bias.detach().float().contiguous(), sc.w_score.weight.detach().float().contiguous())
    for spec in a.attend.split(","):
        Un, W = (int(x) for x in spec.split("x"))
        S = Un * PER_UTT
        nb = S * W
        Ts = torch.randint(T_MIN, T_MAX + 1, (Un,), generator=g).tolist()
        Ts[0] = T_MAX
        moff, offs = ops.las_group_offsets(Ts, dev)
        sutt_host = [u for u in range(Un) for _ in range(PER_UTT)]
        sutt = ops.las_cells_map(sutt_host, Un, dev)
        pk = torch.randn(offs[-1], A, generator=g).to(dev, dt)
        eo = torch.randn(offs[-1], D, generator=g).to(dev, dt)
        rep = lambda x: torch.cat([x[offs[u]:offs[u + 1]] for u in sutt_host]).contiguous()
        pk_rep, eo_rep = rep(pk), rep(eo)
        moff_rep, _ = ops.las_group_offsets([Ts[u] for u in sutt_host], dev)
        pq = torch.randn(nb, A, generator=g).to(dev, dt)
        aw_src = torch.zeros(nb, T_MAX, device=dev)
        for s in range(S):
            T = Ts[sutt_host[s]]
            aw_src[s * W:(s + 1) * W, :T] = torch.softmax(torch.randn(W, T, generator=g), dim=1).to(dev)
        parent = torch.cat([s * W + torch.randperm(W, generator=g) for s in range(S)]).to(torch.int32).to(dev)
        state = torch.tensor([[1, W, 0, 0]] * S, dtype=torch.int32, device=dev)
        aw_dst, scores = torch.zeros(nb, T_MAX, device=dev), torch.zeros(nb, T_MAX, device=dev)
        ctx = torch.zeros(nb, D, device=dev, dtype=dt)
        aw2, sc2, ctx2 = torch.zeros_like(aw_dst), torch.zeros_like(scores), torch.zeros_like(ctx)

        def cells_form():
            with ops.stream_scope(False):
                ops.las_attend_cells(Wt, pk, eo, moff, sutt, pq, aw_src, parent, state, W, aw_dst, ctx, scores)

        def group_form():
            with ops.stream_scope(False):
                ops.las_attend_group(Wt, pk_rep, eo_rep, moff_rep, pq, aw_src, parent, state, W, aw2, ctx2, sc2)

        cells_form(); group_form()
        torch.cuda.synchronize()
        assert torch.equal(aw_dst, aw2) and torch.equal(ctx, ctx2)
        tcell, tgrp = [], []
        for _ in range(a.pairs):
            tcell.append(graph_time(cells_form))
            tgrp.append(graph_time(group_form))
        res["attend"][f"U{Un}_W{W}"] = dict(searches=S, rows=nb, frames=offs[-1], replicated_frames=int(np.sum([Ts[u] for u in sutt_host])),
                                            cells_us=stats(tcell), group_replicated_us=stats(tgrp),
                                            group_over_cells=[round(y / x, 3) for x, y in zip(tcell, tgrp)])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
