"""Measure the batched transducer greedy search in lockstep against the per-utterance greedy search (a measurement, not a gate).

    python tools/rnnt_greedy_bench.py [--dtypes f32,bf16] [--batches 1,16,64] [--frames 1,2,4,8] [--blocks 4,8,16,32]
                                      [--repeats 5] [--utt-form 0] [--label-rate 0.2] [--out FILE]

The L4-sized transducer of bench.py (V = 1000, H = 512, J = 512, two LSTM layers) with seeded random weights, on seeded random
encoder outputs for utterances of 180 .. 300 encoder frames.  Random weights would emit a label at every evaluation, so the blank
entry of the output bias is set (by bisection, once per dtype) to the value at which the greedy search emits --label-rate labels
per frame: the share of blanks is what decides how many steps a window of K frames saves.  For each dtype and batch size B:

  batched search   engine.rnnt_greedy_batch on the B utterances for every K of --frames: the w_enc products, the start, the
                   replays with the polls of the live counter, the download and the unpacking into lists; next to it the STEP LOOP
                   alone (replays and polls, the searches already loaded): its time per step and the number of steps, so that the
                   effect of K reads apart from the launch cost
  utterance form   engine.rnnt_greedy as it stands on the SAME B utterances, one search per utterance (--utt-form N > 0: on the
                   first N only -- not like for like where their labels differ from the batch's; the result says which)

and, at the largest batch and the best K, the step loop for every poll block of --blocks.

Every timing is a host clock around work that ends in a device synchronise, after one warm-up run of the same shape, repeated
--repeats times, the forms alternating; the median is reported per utterance, minimum and maximum next to it.  Prints one JSON
line."""
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


def clock(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def step_loop(eng, st, longest, K, block, bound):
    """the replay loop of engine.rnnt_greedy_batch on loaded searches -> steps"""
    steps, todo = 0, -(-longest // K)
    while True:
        for _ in range(todo):
            st.graph.replay()
        steps += todo
        if int(st.live.item()) == 0:
            return steps
        todo = min(block, bound - steps)
        assert todo > 0, (steps, bound)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", type=str, default="f32,bf16")
    ap.add_argument("--batches", type=str, default="1,16,64")
    ap.add_argument("--frames", type=str, default="1,2,4,8")
    ap.add_argument("--blocks", type=str, default="4,8,16,32")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--utt-form", type=int, default=0, help="0: the utterance form on all B utterances")
    ap.add_argument("--label-rate", type=float, default=0.2)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    import bench
    from emoasr_amd.hostenv import respect_cpu_quota
    from emoasr_amd.modeling.asr import ASR
    if not torch.cuda.is_available():
        raise SystemExit("rnnt_greedy_bench: no GPU (there is nothing to measure on the host alone)")
    respect_cpu_quota()
    dev, sync = torch.device("cuda"), torch.cuda.synchronize
    batches = [int(b) for b in args.batches.split(",")]
    Ks = [int(k) for k in args.frames.split(",")]
    blocks = [int(b) for b in args.blocks.split(",")]
    rng = np.random.default_rng(0)
    lens_all = [int(n) for n in rng.integers(180, 301, max(batches))]
    g = torch.Generator().manual_seed(0)
    eouts_f32 = torch.randn(max(batches), 300, bench.L4["enc_hidden_size"], generator=g)
    result = {"device": torch.cuda.get_device_name(0), "model": "L4 (V=1000, H=512, J=512, 2 layers)", "frames": "180..300",
              "label_rate_target": args.label_rate, "poll_block": None, "cases": [], "poll_blocks": []}
    msl = 256
    with torch.no_grad():
        for name in args.dtypes.split(","):
            dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[name]
            torch.manual_seed(2)
            model = ASR(SimpleNamespace(**bench.L4), compute_dtype=dtype).to(dev).eval()
            eng = model.engine()
            eng.ensure_bound()
            blank, eos = model.decoder.blank_id, model.decoder.eos_id
            result["poll_block"] = eng._GREEDY_BATCH_POLL
            eouts_all = eouts_f32.to(dev, dtype)
            # the blank bias at which the search emits label_rate labels per frame (bisection on 8 utterances)
            lo, hi, nb = -20.0, 20.0, min(8, max(batches))
            for _ in range(12):
                mid = 0.5 * (lo + hi)
                model.decoder.output.bias.data[blank] = mid
                hyps, _ = eng.rnnt_greedy_batch(eouts_all[:nb], lens_all[:nb], blank, eos, msl)
                rate = sum(len(h) for h in hyps) / sum(lens_all[:nb])
                lo, hi = (mid, hi) if rate > args.label_rate else (lo, mid)
            print(f"{name}: blank bias {mid:.3f}, {rate:.3f} labels per frame", file=sys.stderr, flush=True)
            for B in batches:
                lens, eouts = lens_all[:B], eouts_all[:B]
                nu = B if args.utt_form <= 0 else min(B, args.utt_form)
                forms = {"utterance": lambda: eng.rnnt_greedy(eouts[:nu], lens[:nu], blank, eos, msl)}
                for K in Ks:
                    forms[f"K{K}"] = lambda K=K: eng.rnnt_greedy_batch(eouts, lens, blank, eos, msl, frames_per_step=K)
                samples, outs = {k: [] for k in forms}, {}
                for k, fn in forms.items():     # warm-up: code objects, allocator, graph captures
                    outs[k] = fn()
                sync()
                for _ in range(args.repeats):   # the forms alternate, repeat by repeat: all see the same box at the same time
                    for k, fn in forms.items():
                        samples[k].append(clock(fn, sync)[0])
                case = {"dtype": name, "B": B, "frames_mean": sum(lens) / B, "labels_mean": sum(len(h) for h in outs[f"K{Ks[0]}"][0]) / B,
                        "utterance_form": per_utt(samples["utterance"], nu), "utterance_form_utts": nu,
                        "utterance_form_labels_mean": sum(len(h) for h in outs["utterance"][0]) / nu, "batch": []}
                for K in Ks:
                    same = sum(int(a == b) for a, b in zip(outs[f"K{K}"][0][:nu], outs["utterance"][0]))
                    bound = max(lens) + msl + 1
                    loop = []
                    for _ in range(args.repeats + 1):
                        with eng._scope():
                            st = eng._rnnt_greedy_batch_load(eouts, lens, K, blank, eos, msl)
                            dt_, steps = clock(lambda: step_loop(eng, st, max(lens), K, eng._GREEDY_BATCH_POLL, bound), sync)
                        loop.append(dt_)
                    loop = loop[1:]
                    case["batch"].append({"K": K, **per_utt(samples[f"K{K}"], B), "steps": steps,
                                          "step_us": {"median": 1e6 * statistics.median(loop) / steps, "min": 1e6 * min(loop) / steps,
                                                      "max": 1e6 * max(loop) / steps},
                                          "hyps_equal_utterance_form": f"{same}/{nu}"})
                    print(f"{name} B={B} K={K}: {case['batch'][-1]['median_ms_per_utt']:.3f} ms/utt, {steps} steps of "
                          f"{case['batch'][-1]['step_us']['median']:.1f} us; utterance form "
                          f"{case['utterance_form']['median_ms_per_utt']:.3f} ms/utt", file=sys.stderr, flush=True)
                result["cases"].append(case)
            # the poll block, at the largest batch and the K with the best median there
            B = max(batches)
            lens, eouts = lens_all[:B], eouts_all[:B]
            best = min(result["cases"][-1]["batch"], key=lambda c: c["median_ms_per_utt"])["K"]
            bound = max(lens) + msl + 1
            for block in blocks:
                loop = []
                for _ in range(args.repeats + 1):
                    with eng._scope():
                        st = eng._rnnt_greedy_batch_load(eouts, lens, best, blank, eos, msl)
                        dt_, steps = clock(lambda: step_loop(eng, st, max(lens), best, block, bound), sync)
                    loop.append(dt_)
                loop = loop[1:]
                result["poll_blocks"].append({"dtype": name, "B": B, "K": best, "block": block, "steps_replayed": steps,
                                              "loop_ms": {"median": 1e3 * statistics.median(loop), "min": 1e3 * min(loop),
                                                          "max": 1e3 * max(loop)}})
                print(json.dumps(result["poll_blocks"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
