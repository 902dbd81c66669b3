"""Measure the batched joint CTC / attention beam search against the single device search looped over the same utterances
(a measurement, not a gate).

    python tools/joint_beam_bench.py [--beams 4,10] [--batches 1,16,64] [--repeats 5] [--single-utts 4] [--steps 36] [--out FILE]

The Transformer-decoder model of bench.py's config 4 (`L3`: V = 10000, dd = 256, 4 heads, 6 layers; the 12-layer LM `LM12`; bf16)
with seeded random weights, on seeded random encoder outputs for utterances of 180 .. 300 encoder frames, decode_ctc_weight 0.3,
with and without the LM (lm_weight 0.3).  With random weights <eos> rarely wins, so max_decode_ylen is set to --steps (bench.py's
config 4 decodes 36 steps per utterance for the same reason) and the table says how many steps each search ran: this times
steps, not accuracy.  For each beam width W and batch size B, in one process:

  batched search  decoder.decode on the B utterances (modeling/beam_search_device.py:joint_beam_search_device_batch)
  single search   decoder.decode on the first --single-utts of the same utterances, one after the other
                  (joint_beam_search_device, the form of the parent commit, in its default configuration)

alternating the two forms repeat by repeat; the median per utterance is reported with minimum and maximum.

And the grouped cross-attention kernel alone (emoasr_attn_step_group, the memory stored once per search) against
emoasr_attn_fwd with Tq = 1 on the memory replicated per beam, same inputs, bf16, dd = 256, 4 heads: 20 calls captured into a
graph so that no host time is in the figure, microseconds per call.

    python tools/joint_beam_bench.py --lm rnn [--beams 4,10] [--batches 1,16,64] [--repeats 5] [--steps 36] [--rows 16,160,640]

The same model with the RNN LM of tools/rnnt_fusion_bench.py (2 layers, E = H = 512, V = 10000, bf16, random weights), lm_weight 0.3
(DESIGN.md section 26).  For each W and B, on the SAME B utterances in one process, alternating repeat by repeat:

  device form     decoder.joint_rnnlm_impl = "device": the LM stepped inside the batched device search
  host form       decoder.joint_rnnlm_impl = "host" (the default): one joint_beam_search with the host bookkeeping per utterance

And emoasr_rnnlm_step_rows alone at --rows rows against lm._step_chain (the ordinary products, which also form the log-softmax) on
the same rows, 20 calls captured into a graph, microseconds per call.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(samples, per):
    return {"median": 1e3 * statistics.median(samples) / per, "min": 1e3 * min(samples) / per, "max": 1e3 * max(samples) / per,
            "n": len(samples)}


def attention_forms(torch, ops, dev, S, W, T, repeats, sync, dd=256, H=4, calls=20):
    """us per call: grouped kernel on [S * T, 2 dd] / emoasr_attn_fwd on the replica [S * W, T, 2 dd]"""
    g = torch.Generator().manual_seed(S * 100000 + W * 1000 + T)
    q = torch.randn(S * W, dd, generator=g).to(dev, torch.bfloat16)
    kv = torch.randn(S * T, 2 * dd, generator=g).to(dev, torch.bfloat16)
    moff = torch.arange(S + 1, dtype=torch.int32, device=dev) * T
    rep = kv.view(S, 1, T, 2 * dd).expand(S, W, T, 2 * dd).reshape(S * W, T, 2 * dd).contiguous()
    klens = torch.full((S * W,), T, dtype=torch.int32, device=dev)
    forms = {"grouped_us": lambda: ops.attn_step_group(q, kv, moff, W, H),
             "replicated_us": lambda: ops.attn_fwd(q.view(S * W, 1, dd), rep[..., :dd], rep[..., dd:], H, (dd // H) ** -0.5, klens=klens)}
    out = {}
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
        s = []
        for _ in range(repeats):
            sync()
            t0 = time.perf_counter()
            graph.replay()
            sync()
            s.append(time.perf_counter() - t0)
        out[name] = {"median": 1e6 * statistics.median(s) / calls, "min": 1e6 * min(s) / calls, "max": 1e6 * max(s) / calls}
        del graph
    return out


def rnnlm_step_forms(torch, ops, dev, lm, R, repeats, sync, calls=20):
    """us per call on R rows: emoasr_rnnlm_step_rows / lm._step_chain (both read half 0 of a pool of 2 R slots and write half 1)"""
    g = torch.Generator().manual_seed(R)
    pools = lm.new_pools(2 * R, R)
    pools.ph.copy_(torch.randn(lm.L, 2 * R, lm.H, generator=g).mul(0.5))
    pools.pc.copy_(torch.randn(lm.L, 2 * R, lm.H, generator=g))
    i32 = lambda t: t.to(torch.int32).to(dev)
    ids, parent = i32(torch.randint(3, lm.V, (R,), generator=g)), i32(torch.randint(0, R, (R,), generator=g))
    dst = i32(R + torch.arange(R))
    A = lm._arena
    ws = [lm._w(l) for l in range(lm.L)]
    W = ops.RnnlmStepWeights(A.w("lm.embed.weight"), [w[0] for w in ws], [w[1] for w in ws], lm._bias, A.w("lm.output.weight"),
                             A.p("lm.output.bias"))
    logits = torch.zeros(R, lm.V, device=dev)
    forms = {"step_rows_us": lambda: ops.rnnlm_step_rows(W, R, ids, parent, pools.ph, pools.pc, 0, R, logits),
             "step_chain_us": lambda: lm._step_chain(pools, R, ids, parent, dst, None)}
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
    return {name: {"median": 1e6 * statistics.median(v) / calls, "min": 1e6 * min(v) / calls, "max": 1e6 * max(v) / calls}
            for name, v in samples.items()}


def rnn_main(args):
    """--lm rnn: the device form against the host form of the RNN-LM fusion"""
    import torch
    import bench
    from emoasr_amd import ops
    from emoasr_amd.hostenv import respect_cpu_quota
    from emoasr_amd.modeling import beam_search_device as bsd
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.lm import LM
    if not torch.cuda.is_available():
        raise SystemExit("joint_beam_bench: no GPU (there is nothing to measure on the host alone)")
    respect_cpu_quota()
    dev, sync = torch.device("cuda"), torch.cuda.synchronize
    torch.manual_seed(3)
    model = ASR(SimpleNamespace(**bench.L3), compute_dtype=torch.bfloat16).to(dev).eval()
    V = bench.L3["vocab_size"]
    lm = LM(SimpleNamespace(lm_type="rnn", vocab_size=V, embedding_size=512, hidden_size=512, num_layers=2, dropout_rate=0.0,
                            tie_weights=False), compute_dtype=torch.bfloat16).to(dev).eval()
    eng = model.engine()
    eng.ensure_bound()
    dec = model.decoder
    dec.max_decode_ylen = args.steps
    batches = [int(b) for b in args.batches.split(",")]
    rng = np.random.default_rng(0)
    lens_all = [int(n) for n in rng.integers(180, 301, max(batches))]
    g = torch.Generator().manual_seed(0)
    eouts_all = torch.randn(max(batches), 300, bench.L3["enc_hidden_size"], generator=g).to(dev, torch.bfloat16)
    result = {"device": torch.cuda.get_device_name(0),
              "model": f"bench.py L3 (V={V}, dd=256, 4 heads, 6 layers) + RNN LM (2 layers, E=H=512), bf16, random weights",
              "frames": "180..300", "decode_ctc_weight": 0.3, "lm_weight": 0.3, "max_decode_ylen": args.steps, "cases": [], "step": []}
    with torch.no_grad():
        kw = dict(len_weight=0.0, lm=lm, lm_weight=0.3, decode_ctc_weight=0.3)
        for W in [int(w) for w in args.beams.split(",")]:
            why = bsd.batch_rnnlm_why_not(dec, W, lm, 0.3)
            if why is not None:
                raise SystemExit(f"joint_beam_bench: the device form does not take W = {W}: {why}")
            for B in batches:
                lens, eouts = lens_all[:B], eouts_all[:B]
                box = {}

                def device():
                    dec.joint_beam_impl, dec.joint_rnnlm_impl = "batch", "device"
                    box["d"] = dec.decode(eouts, lens, None, beam_width=W, **kw)
                    dec.joint_beam_impl, dec.joint_rnnlm_impl = "single", "host"

                def host():
                    dec.joint_beam_impl = "batch"       # (one utterance too goes through joint_beam_search_batch's loop)
                    box["h"] = dec.decode(eouts, lens, None, beam_width=W, **kw)
                    dec.joint_beam_impl = "single"

                device(), host(), sync()         # warm-up: code objects, allocator, graph captures
                eng._beam_batch_stats = None
                d_s, h_s = [], []
                for _ in range(args.repeats):    # alternate the two forms, repeat by repeat
                    for fn, samples in ((device, d_s), (host, h_s)):
                        sync()
                        t0 = time.perf_counter()
                        fn()
                        sync()
                        samples.append(time.perf_counter() - t0)
                bst = eng._beam_batch_stats
                dm, hm = statistics.median(d_s) / B, statistics.median(h_s) / B
                hd = box["d"][0] if B > 1 else [box["d"][0]]
                hh = box["h"][0] if B > 1 else [box["h"][0]]
                same = sum(1 for a, c in zip(hd, hh) if a[:1] == c[:1])
                case = {"W": W, "B": B, "frames_mean": sum(lens) / B, "device_ms_per_utt": spread(d_s, B), "host_ms_per_utt": spread(h_s, B),
                        "device_steps_per_call": bst["steps"] / bst["calls"], "host_over_device": hm / dm,
                        "device_beyond_the_spread": max(d_s) < min(h_s), "same_best_hypothesis": f"{same} / {B}"}
                print(f"rnn lm W={W} B={B} device {1e3 * dm:.2f} ms/utt ({1e3 * min(d_s) / B:.2f}-{1e3 * max(d_s) / B:.2f}) host {1e3 * hm:.2f} "
                      f"ms/utt ({1e3 * min(h_s) / B:.2f}-{1e3 * max(h_s) / B:.2f}) x{hm / dm:.1f}", file=sys.stderr, flush=True)
                result["cases"].append(case)
        for R in [int(v) for v in args.rows.split(",")]:
            result["step"].append(dict(rows=R, **rnnlm_step_forms(torch, ops, dev, lm, R, max(args.repeats, 5), sync)))
            print(json.dumps(result["step"][-1]), file=sys.stderr, flush=True)
    return result


def emit(result, out):
    line = json.dumps(result)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", type=str, default="4,10")
    ap.add_argument("--batches", type=str, default="1,16,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--single-utts", type=int, default=4)
    ap.add_argument("--steps", type=int, default=36)
    ap.add_argument("--attn-T", type=str, default="64,300,1000")
    ap.add_argument("--attn-W", type=str, default="4,10,16")
    ap.add_argument("--attn-S", type=str, default="1,16,64")
    ap.add_argument("--lm", type=str, default="transformer", choices=["transformer", "rnn"])
    ap.add_argument("--rows", type=str, default="16,160,640", help="--lm rnn: rows of the step kernel's own timing")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.lm == "rnn":
        return emit(rnn_main(args), args.out)
    import torch
    import bench
    from emoasr_amd import ops
    from emoasr_amd.hostenv import respect_cpu_quota
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.lm import LM
    if not torch.cuda.is_available():
        raise SystemExit("joint_beam_bench: no GPU (there is nothing to measure on the host alone)")
    respect_cpu_quota()
    dev, sync = torch.device("cuda"), torch.cuda.synchronize
    torch.manual_seed(3)
    model = ASR(SimpleNamespace(**bench.L3), compute_dtype=torch.bfloat16).to(dev).eval()
    lm = LM(SimpleNamespace(**bench.LM12), compute_dtype=torch.bfloat16).to(dev).eval()
    eng = model.engine()
    eng.ensure_bound()
    dec = model.decoder
    dec.max_decode_ylen = args.steps
    batches = [int(b) for b in args.batches.split(",")]
    rng = np.random.default_rng(0)
    lens_all = [int(n) for n in rng.integers(180, 301, max(batches))]
    g = torch.Generator().manual_seed(0)
    eouts_all = torch.randn(max(batches), 300, bench.L3["enc_hidden_size"], generator=g).to(dev, torch.bfloat16)
    result = {"device": torch.cuda.get_device_name(0),
              "model": "bench.py L3 (V=10000, dd=256, 4 heads, 6 layers) + LM12 (12 layers, d=256), bf16, random weights",
              "frames": "180..300", "decode_ctc_weight": 0.3, "lm_weight_when_on": 0.3, "max_decode_ylen": args.steps,
              "cases": [], "attention": []}
    with torch.no_grad():
        for use_lm in (False, True):
            kw = dict(len_weight=0.0, lm=lm if use_lm else None, lm_weight=0.3 if use_lm else 0.0, decode_ctc_weight=0.3)
            for W in [int(w) for w in args.beams.split(",")]:
                for B in batches:
                    lens, eouts = lens_all[:B], eouts_all[:B]
                    ns = min(B, args.single_utts)
                    box = {}

                    def batched():
                        dec.joint_beam_impl = "batch"
                        box["b"] = dec.decode(eouts, lens, None, beam_width=W, **kw)
                        dec.joint_beam_impl = "single"

                    def single():
                        box["s"] = [dec.decode(eouts[b:b + 1, :lens[b]], lens[b:b + 1], None, beam_width=W, **kw) for b in range(ns)]

                    batched(), single(), sync()      # warm-up: code objects, allocator, graph captures
                    eng._beam_batch_stats = None
                    eng._beam_stats = None
                    b_s, s_s = [], []
                    for _ in range(args.repeats):   # alternate the two forms, repeat by repeat
                        for fn, samples in ((batched, b_s), (single, s_s)):
                            sync()
                            t0 = time.perf_counter()
                            fn()
                            sync()
                            samples.append(time.perf_counter() - t0)
                    bst, sst = eng._beam_batch_stats, eng._beam_stats
                    steps_b = bst["steps"] / bst["calls"]                  # lockstep: steps of the longest search of a chunk
                    steps_s = sst["steps"] / max(sst["utts"], 1)
                    bm, sm = statistics.median(b_s) / B, statistics.median(s_s) / ns
                    case = {"lm": use_lm, "W": W, "B": B, "frames_mean": sum(lens) / B, "single_utts": ns,
                            "batched_ms_per_utt": spread(b_s, B), "single_ms_per_utt": spread(s_s, ns),
                            "batched_steps_per_call": steps_b, "single_steps_per_utt": steps_s,
                            "batched_ms_per_utt_step": 1e3 * bm / steps_b, "single_ms_per_utt_step": 1e3 * sm / steps_s,
                            "single_over_batched": sm / bm}
                    if B == 1:
                        hb, hs = box["b"][0], box["s"][0][0]
                        case["results"] = {"batched": len(hb), "single": len(hs), "best_equal": bool(hb and hs and hb[0] == hs[0])}
                    print(f"lm={use_lm} W={W} B={B} batched {1e3 * bm:.2f} ms/utt ({steps_b:.0f} steps) single {1e3 * sm:.2f} ms/utt "
                          f"({steps_s:.0f} steps) x{sm / bm:.1f}", file=sys.stderr, flush=True)
                    result["cases"].append(case)
        for T in [int(v) for v in args.attn_T.split(",")]:
            for W in [int(v) for v in args.attn_W.split(",")]:
                for S in [int(v) for v in args.attn_S.split(",")]:
                    result["attention"].append(dict(T=T, W=W, S=S, **attention_forms(torch, ops, dev, S, W, T, args.repeats, sync)))
                    print(json.dumps(result["attention"][-1]), file=sys.stderr, flush=True)
    emit(result, args.out)


if __name__ == "__main__":
    main()
