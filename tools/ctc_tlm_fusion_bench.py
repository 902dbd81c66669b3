"""Measure Transformer-LM shallow fusion over a prefix tree in the fused CTC beam search: a measurement, not a
gate.

    python tools/ctc_tlm_fusion_bench.py [--frames 300] [--vocab 10000] [--hidden 256] [--beam 10] [--batches 1,8,64] [--lms 2,12]
                                         [--repeats 5] [--host-utts 8] [--grid-utts 16] [--deep-lm-weight 0.02]
                                         [--out profiles/ctc_tlm_fusion_bench.json]

The synthetic sharpened rows and the protocol of tools/ctc_fusion_bench.py (utterances of 0.6 .. 1.0 x `--frames` encoder frames, a
random head of `--vocab` labels with scaled-up logits and a favoured blank; the acoustic side is computed once and is outside every
timing) and the Transformer LM of bench.py's joint-search legs (LM12: V = 10000, d = 256, 4 heads, 12 layers) as well as its 2-layer
twin, bf16, max_seq_len raised to 512 (<eos> and at most one label per frame), seeded random weights.  Per LM and batch size B, ms per
utterance of one (lm_weight, len_weight) = (0.3, 0.0) search per utterance in four forms:

  tree        modeling/ctc_beam_search.py::_search_device_lm with the tree pass (decoder.ctc_tlm_fusion = "device"): per frame one search
              launch, the record count, emoasr_lm_tree_advance_rec + emoasr_lm_tree_step_rows + emoasr_log_softmax_rows_to
  host pass   the same loop with _StatelessPass on the same rows and LM -- the comparator, this repository's code before the tree:
              per frame the records come to the host, the prefixes are rebuilt and padded there, lm.predict re-runs every new
              prefix from its first token.  It batches over the utterances, so it is timed on all B of them.
  rnn fused   the same loop with the RNN LM of tools/ctc_fusion_bench.py (_StatefulPass)
  unfused     _search_device: one launch for the whole batch, no LM

with the nodes the tree took against node_cap, the mean and the longest prefix reached, and whether the tree's hypotheses equal the
host pass's.  Under lm_weight 0.3 the randomly initialised Transformer LM prunes hard and the prefixes stay short, so the largest B is
run once more with `--deep-lm-weight` (tree and host pass only), where they grow long: the tree at depth against a host pass that
really recomputes long prefixes.  The bf16 tree keeps bf16 logits where the host pass forms f32 ones, so hypotheses may differ by
rounding; `f32_check` runs the 2-layer LM in f32 at B = 8 under both weights to tell rounding from error.  Then one instrumented
tree pass per weight at the largest B with a synchronise after each phase of a frame (search launch, count read, advance, step,
soft-max scatter), and the default 11 x 6 grid over --grid-utts utterances in chunks inside the tree's pool
budget, against the host pass timed on 3 cells (first, middle, last) x --host-utts utterances and scaled to all cells and utterances.

Every timing is a host clock around work that ends in a device synchronise, after one warm-up run of the same shape; the forms
alternate repeat by repeat; median, minimum and maximum of --repeats are reported.  No profiler.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RNN_CFG = dict(lm_type="rnn", vocab_size=10000, embedding_size=512, hidden_size=512, num_layers=2, dropout_rate=0.1, tie_weights=False)


def stats(samples, per=1.0, unit="ms_per_utt"):
    return {f"median_{unit}": 1e3 * statistics.median(samples) / per, f"min_{unit}": 1e3 * min(samples) / per,
            f"max_{unit}": 1e3 * max(samples) / per, "n": len(samples)}


def alternate(forms, repeats, sync):
    """forms: {name: fn} -> {name: [seconds]}; one warm-up of each, then the forms in turn, repeat by repeat"""
    for fn in forms.values():
        fn()
    sync()
    out = {name: [] for name in forms}
    for _ in range(repeats):
        for name, fn in forms.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            out[name].append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--batches", type=str, default="1,8,64")
    ap.add_argument("--lms", type=str, default="2,12")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-utts", type=int, default=8)
    ap.add_argument("--grid-utts", type=int, default=16)
    ap.add_argument("--deep-lm-weight", type=float, default=0.02)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch

    import bench
    from emoasr_amd import ops
    from emoasr_amd.hostenv import respect_cpu_quota
    from emoasr_amd.modeling import ctc_beam_search as cbs
    from emoasr_amd.modeling.functions import ctc_tlm_why_not
    from emoasr_amd.modeling.lm import LM
    if not torch.cuda.is_available():
        raise SystemExit("ctc_tlm_fusion_bench: no GPU (there is nothing to measure on the host alone)")
    respect_cpu_quota()
    dev, sync = torch.device("cuda"), torch.cuda.synchronize
    batches = [int(b) for b in args.batches.split(",")]
    V, W, blank, eos = args.vocab, args.beam, 0, 2
    k = min(W, V)
    n_utts = max(batches + [args.grid_utts])
    rng = np.random.default_rng(0)
    lens_all = [int(n) for n in rng.integers(int(0.6 * args.frames), args.frames + 1, n_utts)]
    g = torch.Generator().manual_seed(0)
    x_all = torch.randn(sum(lens_all), args.hidden, generator=g).to(dev, torch.bfloat16)
    w = (torch.randn(V, args.hidden, generator=g) * (6.0 / args.hidden ** 0.5)).to(dev, torch.bfloat16)   # logits ~ N(0, 6^2)
    bias = torch.zeros(V)
    bias[blank] = 20.0    # the blank wins about four frames in ten
    bias = bias.to(dev)
    off_all = [0]
    for n in lens_all:
        off_all.append(off_all[-1] + n)
    logp_all = ops.log_softmax(ops.gemm_nt(x_all, w, bias=bias, out_f32=True))
    top_all = ops.topk(logp_all, k)[1]
    torch.manual_seed(0)
    rlm = LM(SimpleNamespace(**dict(RNN_CFG, vocab_size=V)), compute_dtype=torch.bfloat16).to(dev).eval()
    dec = SimpleNamespace(vocab_size=V)
    result = {"device": torch.cuda.get_device_name(0), "frames_max": args.frames, "vocab": V, "beam": W, "repeats": args.repeats,
              "rnn_lm": dict(RNN_CFG, vocab_size=V), "lms": []}
    pair = [(0.3, 0.0)]

    def run_case(tlm, B, pair, all_forms):
        """-> the case's record: the forms alternating (all_forms: with the RNN-LM fused and the unfused search), the tree's nodes and
        prefix lengths, the tree's hypotheses against the host pass's"""
        box = {}
        row_off = off_all[:B + 1]
        logp, top = logp_all[:row_off[-1]], top_all[:row_off[-1]]

        def tree():
            box["tree"] = cbs._search_device_lm(logp, top, row_off, W, blank, eos, tlm, pair, tree=True)
            box["stats"] = cbs.tree_stats

        def host():
            box["host"] = cbs._search_device_lm(logp, top, row_off, W, blank, eos, tlm, pair)

        def rnn():
            box["rnn"] = cbs._search_device_lm(logp, top, row_off, W, blank, eos, rlm, pair)

        def unfused():
            box["plain"] = cbs._search_device(logp, top, row_off, W, blank, eos, 0.0)

        forms = {"tree": tree, "host_pass": host}
        if all_forms:
            forms.update({"rnn_fused": rnn, "unfused": unfused})
        t = alternate(forms, args.repeats, sync)
        st = {name: stats(v, B) for name, v in t.items()}
        hyps, scores = box["tree"]
        h_hyps, h_scores = box["host"]
        same = sum(hyps[b][0] == h_hyps[b][0] for b in range(B))
        best = sum(hyps[b][0][0] == h_hyps[b][0][0] for b in range(B))
        diff = max([abs(a - c) / max(1.0, abs(c)) for b in range(B) if hyps[b][0] == h_hyps[b][0]
                    for a, c in zip(scores[b][0], h_scores[b][0])] + [0.0])
        lens = [len(h) for b in range(B) for h in hyps[b][0]]
        used = box["stats"]
        return {"B": B, "frames_mean": sum(lens_all[:B]) / B, **st,
                "host_over_tree": st["host_pass"]["median_ms_per_utt"] / st["tree"]["median_ms_per_utt"],
                "tree_max_below_host_min": st["tree"]["max_ms_per_utt"] < st["host_pass"]["min_ms_per_utt"],
                "nodes_mean": sum(used["nodes"]) / B, "nodes_max": max(used["nodes"]), "node_cap": used["node_cap"],
                "prefix_mean_final": sum(lens) / len(lens), "prefix_longest_final": max(lens),
                "prefix_longest_reached": used["longest_prefix"], "lcap": used["lcap"],
                "utterances_with_equal_hypotheses": f"{same}/{B}", "utterances_with_equal_best": f"{best}/{B}",
                "largest_score_difference_where_equal": diff}

    # are differing hypotheses bf16 rounding?  the 2-layer LM in f32, tree against host pass, both weights
    torch.manual_seed(2)
    f32lm = LM(SimpleNamespace(**dict(bench.LM12, vocab_size=V, num_layers=2, max_seq_len=512)), compute_dtype=torch.float32).to(dev).eval()
    result["f32_check"] = [dict(run_case(f32lm, min(8, max(batches)), [(a, 0.0)], False), lm_weight=a) for a in (0.3, args.deep_lm_weight)]
    del f32lm
    for layers in [int(v) for v in args.lms.split(",")]:
        cfg = dict(bench.LM12, vocab_size=V, num_layers=layers, max_seq_len=512)
        torch.manual_seed(layers)
        tlm = LM(SimpleNamespace(**cfg), compute_dtype=torch.bfloat16).to(dev).eval()
        assert ctc_tlm_why_not(dec, tlm) is None, ctc_tlm_why_not(dec, tlm)
        entry = {"lm": cfg, "cases": [run_case(tlm, B, pair, True) for B in batches]}
        # depth: the same search with a small lm_weight, under which the random LM prunes less and the prefixes grow long
        entry["deep_case"] = dict(run_case(tlm, max(batches), [(args.deep_lm_weight, 0.0)], False), lm_weight=args.deep_lm_weight)
        box = {}
        # the per-frame split, one instrumented tree pass at the largest B
        B = max(batches)
        row_off = off_all[:B + 1]
        logp, top = logp_all[:row_off[-1]], top_all[:row_off[-1]]
        T = max(lens_all[:B])

        def split_pass(lm_weight):
            t = {"search_launch": 0.0, "count_read": 0.0, "advance": 0.0, "step": 0.0, "softmax_scatter": 0.0}
            d_off = torch.tensor(row_off, dtype=torch.int32).to(dev)
            utt = torch.arange(B, dtype=torch.int32).to(dev)
            wt = torch.tensor([[lm_weight] * B, [0.0] * B], dtype=torch.float64).to(dev)
            st = ops.ctc_beam_lm_init(d_off, utt, W, eos, T)
            lm_pass = cbs._TreePass(tlm, B, W, st.slots, V, T, wt[0], dev)
            lm_pass(st, int(st.rec_count.item()))
            records = 0
            sync()
            for f in range(T):
                t0 = time.perf_counter()
                ops.ctc_beam_lm_frame(st, f, logp, top, wt[0], wt[1], blank, lm_pass.logp)
                sync()
                t1 = time.perf_counter()
                n = min(int(st.rec_count.item()), lm_pass.tree.rows)
                t2 = time.perf_counter()
                with ops.stream_scope(lm_pass.split):
                    lm_pass.tree.advance_records(st.rec, st.rec_count, lm_pass.lm_weight)
                    sync()
                    t3 = time.perf_counter()
                    logits = lm_pass.step(n)
                    sync()
                    t4 = time.perf_counter()
                    ops.log_softmax_rows_to(logits, n, st.rec[5], lm_pass.logp, V, row_ok=lm_pass.tree.row_node)
                    sync()
                t5 = time.perf_counter()
                for name, v in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                    t[name] += v
                records += n
            return {"B": B, "frames": T, "lm_weight": lm_weight, "records_per_frame": records / T,
                    **{name + "_us_per_frame": 1e6 * v / T for name, v in t.items()}}

        entry["split"] = []
        for a in (0.3, args.deep_lm_weight):
            split_pass(a)          # (warm-up)
            entry["split"].append(split_pass(a))

        # the grid: chunks of utterances inside the tree's pool budget, the rule of ctc_prefix_beam_search_batch_lm
        G = args.grid_utts
        lm_w, len_w = np.arange(0, 1 + 1e-5, 0.1), np.arange(0, 5 + 1e-5, 1)
        cells = [(float(a), float(b)) for a in lm_w for b in len_w]
        per_utt = len(cells) * cbs._tree_bytes(tlm, W, max(lens_all[:G]))
        n_chunk = max(1, min(G, cbs._TLM_POOL_BUDGET // per_utt))

        def grid():
            box["grid"] = []
            for b0 in range(0, G, n_chunk):
                b1 = min(G, b0 + n_chunk)
                off = [o - off_all[b0] for o in off_all[b0:b1 + 1]]
                hyps, _ = cbs._search_device_lm(logp_all[off_all[b0]:off_all[b1]], top_all[off_all[b0]:off_all[b1]], off, W, blank, eos,
                                                tlm, cells, tree=True)
                box["grid"] += hyps

        n_host = min(G, args.host_utts)
        probe = [cells[0], cells[len(cells) // 2], cells[-1]]

        def host_cells():
            box["host_cells"] = cbs._search_device_lm(logp_all[:off_all[n_host]], top_all[:off_all[n_host]], off_all[:n_host + 1], W,
                                                      blank, eos, tlm, probe)[0]

        t = alternate({"grid": grid, "host": host_cells}, args.repeats, sync)
        scale = (len(cells) / len(probe)) * (G / n_host)
        same = sum(box["grid"][b][cells.index(c)] == box["host_cells"][b][i] for i, c in enumerate(probe) for b in range(n_host))
        grid_st, host_st = stats(t["grid"], unit="ms"), stats([s * scale for s in t["host"]], unit="ms")
        entry["grid"] = {"cells": len(cells), "utterances": G, "searches": len(cells) * G, "utterances_per_chunk": n_chunk,
                         "tree_one_pass": grid_st, "host_pass_scaled": host_st,
                         "host_timed": f"{len(probe)} cells x {n_host} utterances in one call, scaled by {scale:g}",
                         "host_over_tree": host_st["median_ms"] / grid_st["median_ms"],
                         "tree_max_below_host_min": grid_st["max_ms"] < host_st["min_ms"],
                         "probe_searches_with_equal_hypotheses": f"{same}/{len(probe) * n_host}"}
        result["lms"].append(entry)
        del tlm
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
