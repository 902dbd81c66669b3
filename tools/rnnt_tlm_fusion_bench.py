"""Measure Transformer-LM shallow fusion over a prefix tree in the transducer beam search: a measurement, not a
gate.

    python tools/rnnt_tlm_fusion_bench.py [--beams 4,10] [--batches 1,16,64] [--lms 12,2] [--repeats 5] [--host-utts 1] [--out FILE]

The L4-sized transducer of bench.py (V = 1000, H = 512, J = 512, two LSTM layers, bf16) and the Transformer LM of bench.py's joint-search
legs (LM12: V = 10000, d = 256, 4 heads, 12 layers) as well as its 2-layer twin, bf16, max_seq_len raised to 1024 (an utterance of 300
frames may grow 601 labels), seeded random weights, seeded random encoder outputs for utterances of 180 .. 300 encoder frames.  For
each LM, beam width and batch size B, in one process:

  tree device    engine.rnnt_beam_search_batch(..., lm=, lm_weights=[0.3], len_weights=[0], tlm_fusion="device") on the B utterances
  (a) host       engine._rnnt_beam_search_chain with the same LM and weight (the host form: lm.predict on the whole prefix of every
                 new hypothesis, the bookkeeping in Python) on the first --host-utts of them
  (b) plain      engine.rnnt_beam_search_batch without an LM on the B utterances
  (c) rnn fused  engine.rnnt_beam_search_batch with the 2-layer RNN LM of tools/rnnt_fusion_bench.py fused on the device

with the nodes every search took against the worst-case bound the pools are sized for.  With seeded random weights the hypotheses of
these searches stay at one to three labels (the blank extension of the shortest hypothesis wins nearly every frame;
longest_hypothesis in the JSON), so the LM sees short prefixes in all four search forms: the searches measure the step's launch chain
and the bookkeeping, not attention at depth.  Depth is what (d) measures, on the kernel alone:
  (d) kernel     emoasr_lm_tree_attn alone (640 rows, d = 256, 4 heads, lists of n random nodes) against emoasr_attn_step on dense
                 caches of the same n positions, microseconds per launch over --kernel-launches launches between two device events.

Every search timing is a host clock around work that ends in a device synchronise, after one warm-up run of the same shape; the forms
alternate repeat by repeat; the median of --repeats is reported per utterance, minimum and maximum next to it.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def per_utt(samples, B):
    return {"median_ms_per_utt": 1e3 * statistics.median(samples) / B, "min_ms_per_utt": 1e3 * min(samples) / B,
            "max_ms_per_utt": 1e3 * max(samples) / B, "n": len(samples)}


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


def kernel_alone(torch, dev, repeats, launches, lengths=(16, 64, 256, 600)):
    """(d): the gathered kernel against the dense one, both bf16, one query per (row, head) over n positions"""
    from emoasr_amd import lm_tree, ops
    S, W, d, H = 64, 10, 256, 4
    R = S * W
    out = []
    g = torch.Generator().manual_seed(1)
    rs = np.random.default_rng(1)
    for n in lengths:
        state = lm_tree.TreeState(S, W, R, n, n, dev)          # one slot per row, S n nodes
        nodes = S * n
        last = rs.permutation(nodes)[:R]          # every row's own node, distinct; its ancestors among the other nodes
        rest = np.setdiff1d(np.arange(nodes), last)
        lanc = np.stack([np.append(rs.permutation(rest)[:n - 1], last[r]) for r in range(R)]).astype(np.int32)
        state.lanc.copy_(torch.from_numpy(lanc))
        state.llen.fill_(n)
        state.row_node.copy_(torch.from_numpy(lanc[:, n - 1].copy()))
        dst = torch.arange(R, dtype=torch.int64, device=dev)
        qkv = torch.randn(R, 3 * d, generator=g).to(dev, torch.bfloat16)
        kp, vp = (torch.randn(nodes, d, generator=g).to(dev, torch.bfloat16) for _ in range(2))
        kc, vc = (torch.randn(R, n, d, generator=g).to(dev, torch.bfloat16) for _ in range(2))
        pos = torch.tensor([n - 1], dtype=torch.int32, device=dev)
        o = torch.zeros(R, d, device=dev, dtype=torch.bfloat16)
        forms = {"gathered_us": lambda: state.attn(qkv, kp, vp, dst, H, out=o), "dense_us": lambda: ops.attn_step(qkv, kc, vc, pos, H)}
        samples = {k: [] for k in forms}
        for fn in forms.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(repeats):
            for name, fn in forms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(launches):
                    fn()
                b.record()
                b.synchronize()
                samples[name].append(1e3 * a.elapsed_time(b) / launches)
        row = {"rows": R, "d": d, "heads": H, "positions": n, "launches_per_sample": launches}
        for name, v in samples.items():
            row[name] = {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}
        row["gathered_over_dense"] = row["gathered_us"]["median"] / row["dense_us"]["median"]
        print(f"kernel n={n}: gathered {row['gathered_us']['median']:.1f} us, dense {row['dense_us']['median']:.1f} us", file=sys.stderr,
              flush=True)
        out.append(row)
    return out


def save(result, path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(result) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", type=str, default="4,10")
    ap.add_argument("--batches", type=str, default="1,16,64")
    ap.add_argument("--lms", type=str, default="12,2")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-utts", type=int, default=1)
    ap.add_argument("--kernel-launches", type=int, default=200)
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    import bench
    from emoasr_amd.hostenv import respect_cpu_quota
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.lm import LM
    if not torch.cuda.is_available():
        raise SystemExit("rnnt_tlm_fusion_bench: no GPU (there is nothing to measure on the host alone)")
    respect_cpu_quota()
    dev, sync = torch.device("cuda"), torch.cuda.synchronize
    torch.manual_seed(2)
    V = bench.L4["vocab_size"]
    rlm = LM(SimpleNamespace(lm_type="rnn", vocab_size=V, embedding_size=512, hidden_size=512, num_layers=2, dropout_rate=0.0,
                             tie_weights=False), compute_dtype=torch.bfloat16).to(dev).eval()
    model = ASR(SimpleNamespace(**bench.L4), compute_dtype=torch.bfloat16).to(dev).eval()
    eng, blank, eos = model.engine(), model.decoder.blank_id, model.decoder.eos_id
    eng.ensure_bound()
    beams, batches = [int(w) for w in args.beams.split(",")], [int(b) for b in args.batches.split(",")]
    nmax = max(batches)
    lens_all = [int(n) for n in np.random.default_rng(0).integers(180, 301, nmax)]
    g = torch.Generator().manual_seed(0)
    eouts_all = torch.randn(nmax, 300, bench.L4["enc_hidden_size"], generator=g).to(dev, torch.bfloat16)
    mu = args.lm_weight
    result = {"device": torch.cuda.get_device_name(0), "model": "L4 (V=1000, H=512, J=512, 2 layers, bf16)", "frames": "180..300",
              "lm_weight": mu, "rnn_lm": "RNN LM (V=1000, E=512, H=512, 2 layers, bf16)", "cases": [], "kernel_alone": []}
    with torch.no_grad():
        result["kernel_alone"] = kernel_alone(torch, dev, args.repeats, args.kernel_launches)
        for layers in [int(v) for v in args.lms.split(",")]:
            cfg = dict(bench.LM12, num_layers=layers, max_seq_len=1024)
            tlm = LM(SimpleNamespace(**cfg), compute_dtype=torch.bfloat16).to(dev).eval()
            name = f"Transformer LM (V={cfg['vocab_size']}, d={cfg['hidden_size']}, {cfg['num_attention_heads']} heads, {layers} layers, bf16)"
            assert eng.rnnt_beam_tlm_why_not(tlm) is None, eng.rnnt_beam_tlm_why_not(tlm)
            for W in beams:
                for B in batches:
                    lens, eouts = lens_all[:B], eouts_all[:B]
                    nh = min(B, args.host_utts)
                    box = {}
                    forms = {
                        "tree": lambda: box.__setitem__("tree", eng.rnnt_beam_search_batch(eouts, lens, W, blank, eos, lm=tlm,
                                                                                           lm_weights=[mu], len_weights=[0.0],
                                                                                           tlm_fusion="device")),
                        "host": lambda: box.__setitem__("host", [eng._rnnt_beam_search_chain(eouts[b:b + 1, :lens[b]], W, blank, eos, 3,
                                                                                            True, tlm, mu, 0.0) for b in range(nh)]),
                        "plain": lambda: box.__setitem__("plain", eng.rnnt_beam_search_batch(eouts, lens, W, blank, eos)),
                        "rnn": lambda: eng.rnnt_beam_search_batch(eouts, lens, W, blank, eos, lm=rlm, lm_weights=[mu], len_weights=[0.0]),
                    }
                    s = alternate(forms, args.repeats, sync)
                    stats = dict(eng.rnnt_tlm_stats)
                    th = [h[0] for h in box["tree"][0]]
                    same = sum(int(th[b][0] == box["host"][b][0][0]) for b in range(nh))
                    moved = sum(int(th[b][0] != box["plain"][0][b][0]) for b in range(B))
                    tm, hm, pm, rm = (statistics.median(s[k]) / n for k, n in (("tree", B), ("host", nh), ("plain", B), ("rnn", B)))
                    frames = sum(lens) / B
                    bound = [W * 2 * n + 1 for n in lens]
                    longest = max(len(h) for hyps in th for h in hyps)
                    print(f"{layers} layers W={W} B={B} tree {1e3 * tm:.2f} host {1e3 * hm:.2f} plain {1e3 * pm:.2f} rnn "
                          f"{1e3 * rm:.2f} ms/utt, longest hypothesis {longest}", file=sys.stderr, flush=True)
                    result["cases"].append({
                        "lm": name, "lm_layers": layers, "W": W, "B": B, "frames_mean": frames,
                        "tree_device": per_utt(s["tree"], B), "host_form": per_utt(s["host"], nh), "host_utts": nh,
                        "plain_device": per_utt(s["plain"], B), "rnn_fused_device": per_utt(s["rnn"], B), "host_over_tree": hm / tm,
                        "tree_over_plain": tm / pm, "tree_over_rnn_fused": tm / rm, "fusion_us_per_frame": 1e6 * (tm - pm) / frames,
                        "best_hyps_equal_host": f"{same}/{nh}", "best_hyps_moved_by_fusion": f"{moved}/{B}",
                        "longest_hypothesis": longest, "nodes_used_mean": sum(stats["nodes"]) / B, "nodes_used_max": max(stats["nodes"]),
                        "nodes_bound_own_frames_mean": sum(bound) / B, "node_cap_allocated": stats["node_cap"],
                        "list_cap": stats["lcap"], "nodes_used_over_bound": sum(stats["nodes"]) / sum(bound)})
                    save(result, args.out)          # (kept case by case: a run that is cut short leaves what it measured)
            del tlm
    print(json.dumps(result))
    save(result, args.out)


if __name__ == "__main__":
    main()
