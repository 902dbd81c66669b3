"""Measure the batched transducer beam search with the bookkeeping on the device against the search with the host bookkeeping
(a measurement, not a gate).

    python tools/rnnt_beam_bench.py [--beams 4,10] [--batches 1,16,64] [--repeats 5] [--host-utts 4] [--out FILE]

The L4-sized transducer of bench.py (V = 1000, H = 512, J = 512, two LSTM layers, bf16) with seeded random weights, on seeded
random encoder outputs for utterances of 180 .. 300 encoder frames.  For each beam width and batch size B, in one process:

  device search  engine.rnnt_beam_search_batch on the B utterances: w_enc products, start, one graph replay per frame, finish, the
                 one download and the unpacking into lists
  host search    engine._rnnt_beam_search_graph (the default form of a single-utterance decode: the expansion round replayed from a
                 graph, the bookkeeping in Python) on the first --host-utts of the same utterances, one after the other

and, for the LSTM part of a round alone (both layers, R rows): the tiled kernels (emoasr_rnnt_beam_lstm_rows, R / 16 tiles per
launch) against the ordinary products and the cell kernel (engine.rnnt_recurrency on R rows, WITHOUT the state gathers and
scatters a search would add to it), each captured into a graph of 20 steps so that no host time is in the figure.

Every timing is a host clock around work that ends in a device synchronise, after one warm-up run of the same shape, repeated
--repeats times; the median is reported per utterance, minimum and maximum next to it.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from ctypes import c_void_p
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, repeats, sync):
    fn()            # warm-up: code objects, allocator, graph captures
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


def lstm_forms(torch, ops, lib, eng, R, repeats, sync, steps=20):
    """us per step of the two LSTM layers over R rows: tiled kernels / ordinary products + cell kernel"""
    A, H, nl, dev = eng.arena, eng.r_H, eng.r_nl, eng.arena.flat.device
    emb = A.w("decoder.embed.weight")
    g = torch.Generator().manual_seed(R)
    ids = torch.randint(1, emb.shape[0], (R,), generator=g).to(dev)
    src, dst, act = torch.arange(R, device=dev), R + torch.arange(R, device=dev), torch.ones(R, dtype=torch.int64, device=dev)
    ph = [(torch.randn(2 * R, H, generator=g) * 0.3).to(dev, eng.dtype) for _ in range(nl)]
    pc = [(torch.randn(2 * R, H, generator=g) * 0.3).to(dev) for _ in range(nl)]
    bias = [eng._lstm_bias(f"decoder.rnns.{l}").contiguous() for l in range(nl)]
    p = lambda t: c_void_p(t.data_ptr())

    def tiled():
        xtab, ldx, nx, xidx = emb, emb.shape[1], emb.shape[0], ids
        for l in range(nl):
            w_ih, w_hh = A.w(f"decoder.rnns.{l}.weight_ih_l0"), A.w(f"decoder.rnns.{l}.weight_hh_l0")
            lib.call("emoasr_rnnt_beam_lstm_rows", ops.dt(emb), R, w_ih.shape[1], H, p(xtab), ldx, nx, p(xidx), p(w_ih), p(w_hh),
                     p(bias[l]), p(ph[l]), p(pc[l]), 2 * R, p(src), p(dst), p(act), ops._stream())
            xtab, ldx, nx, xidx = ph[l], H, 2 * R, dst

    ids32 = ids.to(torch.int32).view(1, R)
    prev = ([h[:R].contiguous() for h in ph], [c[:R].contiguous() for c in pc])

    def products():
        eng.rnnt_recurrency(ids32, prev, False, False)

    out = {}
    for name, fn in (("tiled_us", tiled), ("products_us", products)):
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), eng._scope():
            fn()
        torch.cuda.current_stream().wait_stream(side)
        sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), eng._scope():
            for _ in range(steps):
                fn()
        s = timed(graph.replay, repeats, sync)
        out[name] = {"median": 1e6 * statistics.median(s) / steps, "min": 1e6 * min(s) / steps, "max": 1e6 * max(s) / steps}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", type=str, default="4,10")
    ap.add_argument("--batches", type=str, default="1,16,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-utts", type=int, default=4)
    ap.add_argument("--lstm-rows", type=str, default="16,64,160,640,1024")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    import bench
    from emoasr_amd import lib, ops
    from emoasr_amd.hostenv import respect_cpu_quota
    from emoasr_amd.modeling.asr import ASR
    if not torch.cuda.is_available():
        raise SystemExit("rnnt_beam_bench: no GPU (there is nothing to measure on the host alone)")
    respect_cpu_quota()
    dev, sync = torch.device("cuda"), torch.cuda.synchronize
    torch.manual_seed(2)
    model = ASR(SimpleNamespace(**bench.L4), compute_dtype=torch.bfloat16).to(dev).eval()
    eng = model.engine()
    eng.ensure_bound()
    blank, eos = model.decoder.blank_id, model.decoder.eos_id
    batches = [int(b) for b in args.batches.split(",")]
    rng = np.random.default_rng(0)
    lens_all = [int(n) for n in rng.integers(180, 301, max(batches))]
    g = torch.Generator().manual_seed(0)
    eouts_all = torch.randn(max(batches), 300, bench.L4["enc_hidden_size"], generator=g).to(dev, torch.bfloat16)
    result = {"device": torch.cuda.get_device_name(0), "model": "L4 (V=1000, H=512, J=512, 2 layers, bf16)", "frames": "180..300",
              "chunk_capacity": eng._BEAM_BATCH_CAP, "cases": [], "lstm_forms": []}
    with torch.no_grad():
        for W in [int(w) for w in args.beams.split(",")]:
            for B in batches:
                lens, eouts = lens_all[:B], eouts_all[:B]
                nh = min(B, args.host_utts)
                box = {}

                def device():
                    box["dev"] = eng.rnnt_beam_search_batch(eouts, lens, W, blank, eos)

                def host():
                    box["host"] = [eng._rnnt_beam_search_graph(eouts[b:b + 1, :lens[b]], W, blank, eos, return_scores=True)
                                   for b in range(nh)]

                # alternate the two forms, repeat by repeat, so that both see the same box at the same time
                device(), host(), sync()
                d_s, h_s = [], []
                for _ in range(args.repeats):
                    for fn, samples in ((device, d_s), (host, h_s)):
                        sync()
                        t0 = time.perf_counter()
                        fn()
                        sync()
                        samples.append(time.perf_counter() - t0)
                hyps, scores = box["dev"]
                same = sum(int(hyps[b][0] == box["host"][b][0][0]) for b in range(nh))
                worst = max(abs(p - q) for b in range(nh) for p, q in zip(scores[b], box["host"][b][1])
                            if hyps[b] == box["host"][b][0]) if any(hyps[b] == box["host"][b][0] for b in range(nh)) else None
                dm, hm = statistics.median(d_s) / B, statistics.median(h_s) / nh
                print(f"W={W} B={B} device {1e3 * dm:.2f} ms/utt host {1e3 * hm:.2f} ms/utt", file=sys.stderr, flush=True)
                result["cases"].append({"W": W, "B": B, "frames_mean": sum(lens) / B, "labels_best_mean": sum(len(h[0]) - 1 for h in hyps) / B,
                                        "device_search": per_utt(d_s, B), "host_search": per_utt(h_s, nh), "host_utts": nh,
                                        "host_over_device": hm / dm, "best_hyps_equal": f"{same}/{nh}",
                                        "largest_score_difference_where_nbest_equal": worst})
        for Rr in [int(r) for r in args.lstm_rows.split(",")]:
            result["lstm_forms"].append(dict(R=Rr, **lstm_forms(torch, ops, lib, eng, Rr, args.repeats, sync)))
            print(json.dumps(result["lstm_forms"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
