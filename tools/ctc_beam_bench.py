"""Measure the batched CTC prefix beam search on the device against the native host loop, no LM (a measurement, not a gate).

    python tools/ctc_beam_bench.py [--frames 300] [--vocab 10000] [--hidden 256] [--beam 10] [--batches 1,8,64] [--repeats 5] [--out FILE]

Synthetic sharpened rows at the LibriSpeech-like shape of the other tools: encoder outputs of `--hidden` units for utterances of
0.6 .. 1.0 x `--frames` frames (12 s of audio at 40 ms per encoder frame), a random head of `--vocab` labels whose logits are
scaled up and whose blank is favoured, as a trained CTC model's are.  For each batch size B, on the same rows in one process:

  acoustic       head product (bf16, f32 logits), log-soft-max and per-frame top-k over all rows of the B utterances: three launches
  device search  emoasr_ctc_beam_batch: one launch for the B utterances, then the one download and the unpacking into lists
                 (`launch` is the launch alone, synchronised; `end_to_end` includes the download and the lists)
  host loop      what decoding one utterance at a time does after the acoustic side: the copy of the utterance's [T, V] rows to
                 the host and one emoasr_ctc_beam_step call per frame (modeling/ctc_beam_search.py: _search_native), B times

Every timing is a host clock around work that ends in a device synchronise, after one warm-up run of the same shape, repeated
`--repeats` times; the median is reported per utterance, minimum and maximum next to it.  Device and host hypotheses are compared.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, repeats, sync):
    fn()            # warm-up: code objects, allocator
    sync()
    out = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return out


def per_utt(samples, B):
    return {"median_ms_per_utt": 1e3 * statistics.median(samples) / B, "min_ms_per_utt": 1e3 * min(samples) / B,
            "max_ms_per_utt": 1e3 * max(samples) / B, "n": len(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--batches", type=str, default="1,8,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    from emoasr_amd import ops
    from emoasr_amd.hostenv import respect_cpu_quota
    from emoasr_amd.modeling import ctc_beam_search as cbs
    if not torch.cuda.is_available():
        raise SystemExit("ctc_beam_bench: no GPU (there is nothing to measure on the host alone)")
    respect_cpu_quota()
    dev, sync = torch.device("cuda"), torch.cuda.synchronize
    batches = [int(b) for b in args.batches.split(",")]
    V, W, blank, eos = args.vocab, args.beam, 0, 2
    k = min(W, V)
    rng = np.random.default_rng(0)
    lens_all = [int(n) for n in rng.integers(int(0.6 * args.frames), args.frames + 1, max(batches))]
    g = torch.Generator().manual_seed(0)
    x_all = torch.randn(sum(lens_all), args.hidden, generator=g).to(dev, torch.bfloat16)
    w = (torch.randn(V, args.hidden, generator=g) * (6.0 / args.hidden ** 0.5)).to(dev, torch.bfloat16)   # logits ~ N(0, 6^2)
    bias = torch.zeros(V)
    bias[blank] = 20.0    # the blank wins about four frames in ten
    bias = bias.to(dev)                   # (the epilogue's bias is f32)
    result = {"device": torch.cuda.get_device_name(0), "frames_max": args.frames, "vocab": V, "beam": W, "cases": []}
    for B in batches:
        lens = lens_all[:B]
        row_off = [0]
        for n in lens:
            row_off.append(row_off[-1] + n)
        x = x_all[:row_off[-1]]
        box = {}

        def acoustic():
            logits = ops.gemm_nt(x, w, bias=bias, out_f32=True)
            box["logp"] = ops.log_softmax(logits)
            box["top"] = ops.topk(box["logp"], k)[1]

        ac_s = timed(acoustic, args.repeats, sync)
        logp, top = box["logp"], box["top"]
        d_off = torch.tensor(row_off, dtype=torch.int32).to(dev)

        def launch():
            box["raw"] = ops.ctc_beam_batch(logp, d_off, top, W, blank, eos, 0.0, max_frames=max(lens))

        def end_to_end():
            box["dev"] = cbs._search_device(logp, top, row_off, W, blank, eos, 0.0)

        def host_loop():
            box["host"] = [cbs._search_native(logp[a:b], top[a:b], b - a, V, k, blank, eos, W, 0.0, None, 0.0)
                           for a, b in zip(row_off[:-1], row_off[1:])]

        la_s = timed(launch, args.repeats, sync)
        ee_s = timed(end_to_end, args.repeats, sync)
        ho_s = timed(host_loop, args.repeats, sync)
        hyps, scores = box["dev"]
        same = all(hyps[b] == box["host"][b][0] for b in range(B))
        worst = max(abs(p - q) / max(1.0, abs(q)) for b in range(B) for p, q in zip(scores[b], box["host"][b][1]))
        labels = [len(h[0]) - 1 for h in hyps]
        result["cases"].append({"B": B, "frames_mean": sum(lens) / B, "labels_best_mean": sum(labels) / B,
                                "acoustic": per_utt(ac_s, B), "device_search_launch": per_utt(la_s, B),
                                "device_search_end_to_end": per_utt(ee_s, B), "host_loop": per_utt(ho_s, B),
                                "host_over_device": statistics.median(ho_s) / statistics.median(ee_s),
                                "hyps_equal": same, "largest_score_difference": worst})
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
