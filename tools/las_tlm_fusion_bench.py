"""Transformer-LM shallow fusion in the LAS beam search: the search with the LM stepped over the prefix tree on the
device (las_tlm_fusion = "device") against the host form per utterance, the RNN-LM fused search and the unfused search; the
(lm_weight, len_weight) grid in one call against one call per cell; and the LM part of one step, launch group by launch group.

    python tools/las_tlm_fusion_bench.py [--pairs 5] [--batches 1,16,64] [--widths 4,10] [--layers 12,2] [--host-utts 8]

Prints one JSON line (and every figure, as it comes, on stderr).  Protocol of tools/las_fusion_bench.py (section 28): tools/las_bench.py's model size in bf16, ragged T 200..400
encoder frames, <eos> suppressed so that every search runs all max_decode_ylen = 60 steps (every prefix reaches depth 60); host time
from the call to the result with the device synchronised; the forms of one row alternate in ONE process; median, min and max over
--pairs.  The Transformer LM is bench.py's LM12 (V = 10000, d = 256, 4 heads, 12 layers) and its 2-layer twin, the RNN LM
tools/las_fusion_bench.py's, seeded random weights.
  search["L{layers}_B{B}_W{W}"]   ms per utterance of LASDecoder.decode on B utterances: `tree` (one batched device search, the LM over
                        the prefix tree), `host` (las_tlm_fusion = "host": one host-form search per utterance, over the first
                        min(B, --host-utts) utterances), `rnn_fused` (the RNN LM inside the chain) and `unfused`; every pair's ratio
                        host / tree.
  grid["L{layers}_B{B}_W{W}"]     s of the default 11 x 6 grid on B utterances: `one_call` (las_fusion_grid_apply: ten fused searches and
                        one unfused per utterance) and `per_cell` = 6 x the timed cell (0, 0) + 30 x the timed cells (0.5, 0) and
                        (1.0, 5) each, every cell ONE batched decode call -- three cells are timed, the other 63 are scaled from them.
  step["L{layers}_B{B}_W{W}_p{p}"]  us of the LM's launches of ONE step with every row alive at prefix position p (1: next to no
                        keys to gather; 59: the deepest step of the search), device time by graph replay (tools/_timing.py):
                        `advance` (emoasr_lm_tree_advance_beam; the difference of two timings, with and without it, around the
                        copy that puts the node counters back), `lm_step` (emoasr_lm_tree_step), `scatter`
                        (emoasr_log_softmax_rows_to) and `scoring` (emoasr_beam_scores_topk).
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from _timing import graph_time  # noqa: E402
from las_bench import CFG, SIZE, U as STEPS  # noqa: E402
from las_fusion_bench import LM_CFG as RNN_CFG, T_MAX, T_MIN, stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--widths", default="4,10")
    ap.add_argument("--layers", default="12,2")
    ap.add_argument("--host-utts", type=int, default=8)
    ap.add_argument("--grid-batch", type=int, default=16)
    ap.add_argument("--grid-widths", default="4,10")
    ap.add_argument("--step-batch", type=int, default=16)
    ap.add_argument("--depths", default="1,59")
    a = ap.parse_args()
    from emoasr_amd import lib, lm_tree, ops
    from emoasr_amd.fusion_grid import weight_lists
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.functions import las_fusion_grid_apply, las_rnnlm_why_not, las_tlm_why_not
    from emoasr_amd.modeling.lm import LM
    dev, dt = torch.device("cuda"), torch.bfloat16
    torch.manual_seed(0)
    model = ASR(SimpleNamespace(**CFG), compute_dtype=dt).to(dev).eval()
    rnn = LM(SimpleNamespace(**RNN_CFG), compute_dtype=dt).to(dev).eval()
    with torch.no_grad():
        model.decoder.output.bias[CFG["eos_id"]] = -1e4    # <eos> never wins: all steps run, with or without the LM
    dec = model.decoder
    assert las_rnnlm_why_not(dec, 10, rnn) is None
    g = torch.Generator().manual_seed(1)
    D, V = SIZE["enc_hidden_size"], SIZE["vocab_size"]
    batches, widths = [int(x) for x in a.batches.split(",")], [int(x) for x in a.widths.split(",")]
    res = {"size": dict(SIZE, T=[T_MIN, T_MAX], U=STEPS), "rnn_lm": RNN_CFG, "dtype": "bf16", "pairs": a.pairs, "host_utts": a.host_utts,
           "lm": {}, "search": {}, "grid": {}, "step": {}}
    data = {}

    def utterances(B):
        if B not in data:
            elens = torch.randint(T_MIN, T_MAX + 1, (B,), generator=g)
            elens[0] = T_MAX
            data[B] = (torch.randn(B, T_MAX, D, generator=g).to(dev, dt), elens.tolist())
        return data[B]

    def decode(eouts, el, W, lm, mode, tlm="host", lw=0.0, a_lm=0.5):
        dec.las_lm_fusion, dec.las_tlm_fusion, dec.las_beam_impl = mode, tlm, "batch"
        try:
            hyps, _, _, _ = dec.decode(eouts, el, None, W, lw, lm=lm, lm_weight=a_lm)
        finally:
            dec.las_lm_fusion, dec.las_tlm_fusion, dec.las_beam_impl = "ignore", "host", "single"
        assert hyps in ([], [[]] * len(el))

    lm_weights, len_weights = weight_lists(0, 1, 0.1, 0, 5, 1)
    assert len(lm_weights) == 11 and len(len_weights) == 6
    for layers in [int(x) for x in a.layers.split(",")]:
        cfg = dict(bench.LM12, num_layers=layers)
        torch.manual_seed(2)
        lm = LM(SimpleNamespace(**cfg), compute_dtype=dt).to(dev).eval()
        assert las_tlm_why_not(dec, 10, lm) is None
        res["lm"][f"L{layers}"] = cfg
        # ---- the searches
        for B in batches:
            eouts, el = utterances(B)
            nh = min(B, a.host_utts)
            for W in widths:
                def host():
                    dec.las_lm_fusion = "fuse"
                    try:
                        for b in range(nh):
                            hyps, _, _, _ = dec.decode(eouts[b:b + 1, :el[b]], [el[b]], None, W, 0.0, lm=lm, lm_weight=0.5)
                            assert hyps == []
                    finally:
                        dec.las_lm_fusion = "ignore"

                forms = dict(tree=(lambda: decode(eouts, el, W, lm, "fuse", "device"), B), host=(host, nh),
                             rnn_fused=(lambda: decode(eouts, el, W, rnn, "fuse"), B), unfused=(lambda: decode(eouts, el, W, lm, "ignore"), B))
                for fn, _ in forms.values():      # warm-up: buffers, the captured steps
                    fn()
                t = {k: [] for k in forms}
                for _ in range(a.pairs):
                    for k, (fn, per) in forms.items():
                        t[k].append(timed(fn, per))
                row = {k + "_ms_per_utt": stats(v) for k, v in t.items()}
                row["host_over_tree"] = [round(y / x, 3) for x, y in zip(t["tree"], t["host"])]
                res["search"][f"L{layers}_B{B}_W{W}"] = row
                print(f"search L{layers} B{B} W{W}: {row}", file=sys.stderr, flush=True)
        # ---- the grid
        B = a.grid_batch
        eouts, el = utterances(B)
        for W in [int(x) for x in a.grid_widths.split(",")]:
            def one_call():
                dec.las_tlm_fusion = "device"
                try:
                    hyps, _ = las_fusion_grid_apply(dec, eouts, el, W, lm, lm_weights, len_weights)
                finally:
                    dec.las_tlm_fusion = "host"
                assert len(hyps) == B and all(len(h) == 66 and not any(h) for h in hyps)

            cells = {"c0_0": lambda: decode(eouts, el, W, lm, "ignore", "device", 0.0, 0.0),
                     "c05_0": lambda: decode(eouts, el, W, lm, "fuse", "device", 0.0, 0.5),
                     "c1_5": lambda: decode(eouts, el, W, lm, "fuse", "device", 5.0, 1.0)}
            one_call()
            for fn in cells.values():
                fn()
            t1, tc = [], {k: [] for k in cells}
            for _ in range(a.pairs):
                t1.append(timed(one_call) / 1e3)
                for k, fn in cells.items():
                    tc[k].append(timed(fn) / 1e3)
            per_cell = [6 * x + 30 * (y + z) for x, y, z in zip(tc["c0_0"], tc["c05_0"], tc["c1_5"])]
            res["grid"][f"L{layers}_B{B}_W{W}"] = dict(one_call_s=stats(t1), per_cell_s=stats(per_cell),
                                                        timed_cells_s={k: stats(v) for k, v in tc.items()},
                                                        per_cell_over_one_call=[round(y / x, 3) for x, y in zip(t1, per_cell)])
            print(f"grid L{layers} B{B} W{W}: {res['grid'][f'L{layers}_B{B}_W{W}']}", file=sys.stderr, flush=True)
        # ---- the LM's launches of one step, every row alive at position p
        S = a.step_batch
        lm._prepare()
        for W in widths:
            nb = S * W
            tree = lm_tree.TreeState(S, W, 2 * nb, lm_tree.las_list_cap(STEPS, cfg["max_seq_len"]), lm_tree.las_node_cap(W, STEPS), dev)
            tstep = lm_tree.TreeStep(lm, tree)
            parent = torch.arange(nb, device=dev, dtype=torch.int32)
            state = torch.tensor([[0, W, 0, 0]] * S, dtype=torch.int32, device=dev)
            head = torch.randn(nb, V, generator=g).to(dev)
            lmrows = torch.zeros(nb, V, device=dev)
            vals, cands = torch.zeros(nb, W, device=dev), torch.zeros(nb, W, device=dev, dtype=torch.int32)
            for p in [int(x) for x in a.depths.split(",")]:
                tree.reset()
                with ops.stream_scope(False):
                    for i in range(p + 1):      # the walk to position p: every row its own child, K / V written on the way
                        ids = torch.randint(3, V, (nb,), generator=g).to(torch.int32).to(dev)
                        tree.advance_beam(ids, parent, state, (i % 2) * nb, (1 - i % 2) * nb)
                        tstep()
                torch.cuda.synchronize()
                assert not tree.status.any() and int(tree.row_pos.min()) == p
                before = tree.nnodes - W          # the node counters before the step at position p
                src, dst = (p % 2) * nb, (1 - p % 2) * nb

                def put_back():      # (the same nodes again: the lists and lengths the step writes are the ones that stand there)
                    tree.nnodes.copy_(before)

                def with_advance():
                    put_back()
                    with ops.stream_scope(False):
                        tree.advance_beam(ids, parent, state, src, dst)

                def lm_step():
                    with ops.stream_scope(False):
                        tstep()

                def scatter():
                    with ops.stream_scope(False):
                        ops.log_softmax_rows_to(tstep.logits, nb, parent, lmrows, V, row_ok=tree.row_node)

                def scoring():
                    lib.call("emoasr_beam_scores_topk", lib.F32, nb, V, W, ops._p(head), V, ops._p(lmrows), V, 0.5, ops._p(vals),
                             ops._p(cands), None, ops._stream())

                t = dict(advance=[], lm_step=[], scatter=[], scoring=[])
                for _ in range(a.pairs):
                    t["advance"].append(graph_time(with_advance) - graph_time(put_back))
                    t["lm_step"].append(graph_time(lm_step))
                    t["scatter"].append(graph_time(scatter))
                    t["scoring"].append(graph_time(scoring))
                with_advance()
                torch.cuda.synchronize()
                assert not tree.status.any() and int(tree.row_pos.min()) == p and int(tree.row_node.min()) >= 0
                res["step"][f"L{layers}_B{S}_W{W}_p{p}"] = {k + "_us": stats(v) for k, v in t.items()}
                print(f"step L{layers} B{S} W{W} p{p}: {res['step'][f'L{layers}_B{S}_W{W}_p{p}']}", file=sys.stderr, flush=True)
            del tstep, tree
    print(json.dumps(res))


if __name__ == "__main__":
    main()
