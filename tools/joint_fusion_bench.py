"""Measure the joint CTC / attention fusion grid against one batched search per cell (a measurement, not a
gate).

    python tools/joint_fusion_bench.py [--repeats 5] [--batch 16] [--beam 10] [--steps 36] [--legs a,b,c,d,e] [--out FILE]

The sizes of tools/joint_beam_bench.py: bench.py's config-4 model (`L3`: V = 10000, dd = 256, 4 heads, 6 layers; the 12-layer LM
`LM12`; bf16) with seeded random weights, B utterances of 180 .. 300 random encoder frames, decode_ctc_weight 0.3, max_decode_ylen
= --steps (with random weights <eos> rarely wins: this times steps, not accuracy), and the reference's default grid: lm_weight
0 .. 1 in steps of 0.1 x len_weight 0 .. 5 in steps of 1 = 11 x 6 cells.  Milliseconds per utterance for

  (a) grid       joint_beam_search_device_grid: one call, 11 searches per utterance;
  (b) per cell   66 calls of joint_beam_search_device_batch over the same encoded batch, one per cell (the form before the grid);
  (c) per weight 11 such calls, one per distinct lm_weight at len_weight 0 -- what de-duplicating len_weight alone buys; the rest of
                 (a) against (c) is what sharing the frames and one launch chain buys;
  (d) emoasr_attn_step_cells alone at 1, 2 and 3 searches per workgroup against emoasr_attn_step_group over the same searches on
      replicated memory, T = 300, 20 calls captured into a graph, microseconds per call: over all B x 10 searches, and over the
      searches of the grid call's largest chunk;
  (e) the grid call with 1 .. 32 // W searches per attention workgroup, in one process, alternating (each timed call follows an untimed one with the same grouping, which re-captures the step graphs).

The legs alternate repeat by repeat; the median is reported with minimum and maximum.  Prints one JSON line.

    python tools/joint_fusion_bench.py --lm rnn [--repeats 5] [--batch 16] [--beam 10] [--steps 36] [--out FILE]

The same grid with the RNN LM of tools/rnnt_fusion_bench.py (2 layers, E = H = 512, bf16, random weights), on
the same utterances in one process, alternating: (device) joint_beam_search_device_grid under decoder.joint_rnnlm_impl = "device" --
one pass, the LM stepped inside the captured chain -- and (host) the same call under the default "host": one host search per utterance
and distinct lm_weight."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(samples, scale):
    return {"median": scale * statistics.median(samples), "min": scale * min(samples), "max": scale * max(samples), "n": len(samples)}


def attention_leg(torch, ops, dev, U, NM, W, T, repeats, sync, dd=256, H=4, calls=20):
    """us per call over U * NM searches of width W: the grouped kernel on memory replicated per search, the cell kernel at 1, 2, 3
    searches per workgroup on the utterances' memory"""
    g = torch.Generator().manual_seed(U * 1000 + NM * 10 + W)
    S = U * NM
    q = torch.randn(S * W, dd, generator=g).to(dev, torch.bfloat16)
    kv = torch.randn(U * T, 2 * dd, generator=g).to(dev, torch.bfloat16)
    moff = torch.arange(U + 1, dtype=torch.int32, device=dev) * T
    sutt = [u for u in range(U) for _ in range(NM)]
    rep = kv.view(U, 1, T, 2 * dd).expand(U, NM, T, 2 * dd).reshape(S * T, 2 * dd).contiguous()
    roff = torch.arange(S + 1, dtype=torch.int32, device=dev) * T
    forms = {"grouped_replicated_us": lambda: ops.attn_step_group(q, rep, roff, W, H)}
    for cpg in (1, 2, 3):
        if cpg * W > 32:
            continue
        groups, most = ops.cell_groups(sutt, W, cpg)
        table = torch.tensor([v for gr in groups for v in gr], dtype=torch.int32).to(dev)
        out = torch.empty_like(q)

        def cells(table=table, G=len(groups), most=most, out=out):
            from emoasr_amd import lib
            lib.call("emoasr_attn_step_cells", ops.dt(q), G, most, S * W, U, dd, H, q.data_ptr(), kv.data_ptr(), moff.data_ptr(),
                     table.data_ptr(), out.data_ptr(), ops._stream())

        forms[f"cells_{cpg}_per_group_us"] = cells
    res = {}
    graphs = {}
    for name, fn in forms.items():
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), ops.stream_scope():
            fn()
        torch.cuda.current_stream().wait_stream(side)
        sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), ops.stream_scope():
            for _ in range(calls):
                fn()
        graph.replay()
        sync()
        graphs[name] = graph
    samples = {name: [] for name in forms}
    for _ in range(repeats):            # alternate the forms, repeat by repeat
        for name, graph in graphs.items():
            sync()
            t0 = time.perf_counter()
            graph.replay()
            sync()
            samples[name].append(time.perf_counter() - t0)
    for name in forms:
        res[name] = spread(samples[name], 1e6 / calls)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--steps", type=int, default=36)
    ap.add_argument("--legs", type=str, default="a,b,c,d,e")
    ap.add_argument("--cells-per-group", type=int, default=None, help="searches per attention workgroup in (a); default: the library's")
    ap.add_argument("--lm", type=str, default="transformer", choices=["transformer", "rnn"])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    import bench
    from emoasr_amd import ops
    from emoasr_amd.fusion_grid import weight_lists
    from emoasr_amd.hostenv import respect_cpu_quota
    from emoasr_amd.modeling import beam_search_device as bsd
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.lm import LM
    if not torch.cuda.is_available():
        raise SystemExit("joint_fusion_bench: no GPU (there is nothing to measure on the host alone)")
    respect_cpu_quota()
    legs = set(args.legs.split(","))
    dev, sync = torch.device("cuda"), torch.cuda.synchronize
    torch.manual_seed(3)
    model = ASR(SimpleNamespace(**bench.L3), compute_dtype=torch.bfloat16).to(dev).eval()
    if args.lm == "rnn":
        lm = LM(SimpleNamespace(lm_type="rnn", vocab_size=bench.L3["vocab_size"], embedding_size=512, hidden_size=512, num_layers=2,
                                dropout_rate=0.0, tie_weights=False), compute_dtype=torch.bfloat16).to(dev).eval()
    else:
        lm = LM(SimpleNamespace(**bench.LM12), compute_dtype=torch.bfloat16).to(dev).eval()
    model.engine().ensure_bound()
    dec = model.decoder
    dec.max_decode_ylen = args.steps
    B, W, lam = args.batch, args.beam, 0.3
    if args.cells_per_group is not None:
        bsd.GRID_CELLS_PER_GROUP = args.cells_per_group
    rng = np.random.default_rng(0)
    lens = [int(n) for n in rng.integers(180, 301, B)]
    g = torch.Generator().manual_seed(0)
    eouts = torch.randn(B, 300, bench.L3["enc_hidden_size"], generator=g).to(dev, torch.bfloat16)
    lm_w, len_w = weight_lists(0, 1, 0.1, 0, 5, 1)
    lm_w, len_w = [float(a) for a in lm_w], [float(b) for b in len_w]
    result = {"device": torch.cuda.get_device_name(0),
              "model": "bench.py L3 (V=10000, dd=256, 4 heads, 6 layers) + LM12 (12 layers, d=256), bf16, random weights",
              "frames": "180..300", "B": B, "W": W, "decode_ctc_weight": lam, "max_decode_ylen": args.steps,
              "grid": f"{len(lm_w)} x {len(len_w)}", "cells_per_group": bsd.GRID_CELLS_PER_GROUP or max(1, 32 // W)}
    box = {}
    if args.lm == "rnn":
        why = bsd.batch_rnnlm_why_not(dec, W, lm, lam)
        if why is not None:
            raise SystemExit(f"joint_fusion_bench: the device form does not take this configuration: {why}")
        result["model"] = "bench.py L3 (V=10000, dd=256, 4 heads, 6 layers) + RNN LM (2 layers, E=H=512), bf16, random weights"

        def form(impl):
            dec.joint_rnnlm_impl = impl
            box[impl] = bsd.joint_beam_search_device_grid(dec, eouts, lens, W, lm, lm_w, len_w, lam)
            dec.joint_rnnlm_impl = "host"

        with torch.no_grad():
            form("device"), form("host"), sync()        # warm-up: code objects, allocator, graph captures
            samples = {"device": [], "host": []}
            for _ in range(args.repeats):
                for impl in ("device", "host"):
                    sync()
                    t0 = time.perf_counter()
                    form(impl)
                    sync()
                    samples[impl].append(time.perf_counter() - t0)
        result["device_grid_ms_per_utt"] = spread(samples["device"], 1e3 / B)
        result["host_grid_ms_per_utt"] = spread(samples["host"], 1e3 / B)
        result["host_over_device"] = statistics.median(samples["host"]) / statistics.median(samples["device"])
        result["device_beyond_the_spread"] = max(samples["device"]) < min(samples["host"])
        n_cells = len(lm_w) * len(len_w)
        same = sum(1 for b in range(B) for c in range(n_cells) if box["device"][0][b][c][:1] == box["host"][0][b][c][:1])
        result["cells_with_the_same_best_hypothesis"] = f"{same} / {B * n_cells}"
        line = json.dumps(result)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return

    def grid():
        box["a"] = bsd.joint_beam_search_device_grid(dec, eouts, lens, W, lm, lm_w, len_w, lam)

    def per_cell():
        box["b"] = [bsd.joint_beam_search_device_batch(dec, eouts, lens, W, w, lm, a, lam)[:2] for a in lm_w for w in len_w]

    def per_weight():
        box["c"] = [bsd.joint_beam_search_device_batch(dec, eouts, lens, W, 0.0, lm, a, lam)[:2] for a in lm_w]

    forms = [(k, fn) for k, fn in (("a", grid), ("b", per_cell), ("c", per_weight)) if k in legs]
    with torch.no_grad():
        for _, fn in forms:         # warm-up: code objects, allocator, graph captures
            fn()
            sync()
        samples = {k: [] for k, _ in forms}
        for _ in range(args.repeats):
            for k, fn in forms:
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                samples[k].append(time.perf_counter() - t0)
        names = {"a": "grid_ms_per_utt", "b": "per_cell_66_calls_ms_per_utt", "c": "per_weight_11_calls_ms_per_utt"}
        for k, _ in forms:
            result[names[k]] = spread(samples[k], 1e3 / B)
        if "a" in box and "b" in box:     # the two forms agree on the best hypothesis of (nearly) every cell: bf16, other row counts
            same = sum(1 for b in range(B) for c in range(len(box["b"]))
                       if (box["a"][0][b][c][:1] == box["b"][c][0][b][:1]))
            result["cells_with_the_same_best_hypothesis"] = f"{same} / {B * len(box['b'])}"
        n_pos = len([a for a in lm_w if a > 0])
        if "d" in legs:
            result["attention_T300"] = attention_leg(torch, ops, dev, B, n_pos, W, 300, max(args.repeats, 5), sync)
            cap = bsd.batch_chunk_capacity(W, args.steps + 1, model.engine().dnl, model.engine().dd, lm.params.num_layers,
                                           lm.params.hidden_size, 2)
            u_chunk = max(len({b for b, _, _ in chunk}) for chunk in bsd.grid_chunk_plan(B, n_pos, cap))
            if u_chunk != B and cap >= n_pos:
                result[f"attention_T300_largest_chunk_{u_chunk}_utts"] = attention_leg(torch, ops, dev, u_chunk, n_pos, W, 300,
                                                                                       max(args.repeats, 5), sync)
        if "e" in legs:
            was = bsd.GRID_CELLS_PER_GROUP
            ab = {c: [] for c in range(1, max(1, 32 // W) + 1)}
            for _ in range(args.repeats):
                for cpg, samples in ab.items():
                    bsd.GRID_CELLS_PER_GROUP = cpg
                    grid()              # (re-captures the step graphs for this grouping)
                    sync()
                    t0 = time.perf_counter()
                    grid()
                    sync()
                    samples.append(time.perf_counter() - t0)
            bsd.GRID_CELLS_PER_GROUP = was
            result["grid_ms_per_utt_by_cells_per_group"] = {str(cpg): spread(v, 1e3 / B) for cpg, v in ab.items()}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
