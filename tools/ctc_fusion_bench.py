"""Measure the batched CTC prefix beam search WITH LM fusion on the device against the native host loop (a measurement, not a gate).

    python tools/ctc_fusion_bench.py [--frames 300] [--vocab 10000] [--hidden 256] [--beam 10] [--batches 1,8,64] [--repeats 5]
                                     [--host-utts 8] [--grid-utts 64] [--out FILE]

The synthetic sharpened rows of tools/ctc_beam_bench.py (utterances of 0.6 .. 1.0 x `--frames` encoder frames, a random head of
`--vocab` labels with scaled-up logits and a favoured blank) and a randomly initialised RNN LM of the size tools/rnnlm_bench.py
measures (vocabulary 10 000, embedding 512, 2 layers of 512 units, bf16).  The acoustic side (head, log-soft-max, top-k) is computed
once and is outside every timing: both paths start from the same logp / top rows on the device.

  device fused search  modeling/ctc_beam_search.py: _search_device_lm, one (lm_weight, len_weight) = (0.3, 0.0) pair: pools, init, per
                       frame one emoasr_ctc_beam_lm_frame launch + the record count + the LM steps, finish, the one download and
                       the lists -- for the B utterances together
  host loop            the parent's path for the same work: _search_native with the same LM, one utterance at a time (copy of the
                       rows to the host, per frame one C call, one LM call for the new prefixes, one [live, k] gather and one
                       download).  Utterances are independent there, so it is timed on the first min(B, --host-utts) utterances
                       and reported per utterance.
  grid                 the default 11 x 6 = 66 cells (np.arange(0, 1 + 1e-5, 0.1) x np.arange(0, 5 + 1e-5, 1)) over --grid-utts
                       utterances in ONE device pass, against the host loop timed on 3 cells (first, middle, last) x --host-utts
                       utterances and scaled to 66 cells x --grid-utts utterances
  split                one instrumented device pass at the largest B with a synchronise after each phase of a frame: search
                       launch, record-count download, LM steps

Every timing is a host clock around work that ends in a device synchronise, after one warm-up run of the same shape, repeated
`--repeats` times in one process; median, minimum and maximum are reported.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LM_CFG = dict(lm_type="rnn", vocab_size=10000, embedding_size=512, hidden_size=512, num_layers=2, dropout_rate=0.1, tie_weights=False)


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


def stats(samples, per=1.0, unit="ms_per_utt"):
    return {f"median_{unit}": 1e3 * statistics.median(samples) / per, f"min_{unit}": 1e3 * min(samples) / per,
            f"max_{unit}": 1e3 * max(samples) / per, "n": len(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--batches", type=str, default="1,8,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-utts", type=int, default=8)
    ap.add_argument("--grid-utts", type=int, default=64)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    from emoasr_amd import ops
    from emoasr_amd.hostenv import respect_cpu_quota
    from emoasr_amd.modeling import ctc_beam_search as cbs
    from emoasr_amd.modeling.lm import LM
    if not torch.cuda.is_available():
        raise SystemExit("ctc_fusion_bench: no GPU (there is nothing to measure on the host alone)")
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
    torch.manual_seed(0)
    lm = LM(SimpleNamespace(**dict(LM_CFG, vocab_size=V)), compute_dtype=torch.bfloat16).to(dev).eval()
    off_all = [0]
    for n in lens_all:
        off_all.append(off_all[-1] + n)
    logp_all = ops.log_softmax(ops.gemm_nt(x_all, w, bias=bias, out_f32=True))
    top_all = ops.topk(logp_all, k)[1]
    result = {"device": torch.cuda.get_device_name(0), "frames_max": args.frames, "vocab": V, "beam": W, "lm": dict(LM_CFG, vocab_size=V),
              "repeats": args.repeats, "cases": []}
    box = {}

    def host_loop(n_host, lm_weight, len_weight):
        box["host"] = [cbs._search_native(logp_all[a:b], top_all[a:b], b - a, V, k, blank, eos, W, len_weight, lm, lm_weight)
                       for a, b in zip(off_all[:n_host], off_all[1:n_host + 1])]

    for B in batches:
        row_off = off_all[:B + 1]
        logp, top = logp_all[:row_off[-1]], top_all[:row_off[-1]]
        n_host = min(B, args.host_utts)

        def device():
            box["dev"] = cbs._search_device_lm(logp, top, row_off, W, blank, eos, lm, [(0.3, 0.0)])

        de_s = timed(device, args.repeats, sync)
        ho_s = timed(lambda: host_loop(n_host, 0.3, 0.0), args.repeats, sync)
        hyps, scores = box["dev"]
        same = sum(hyps[b][0] == box["host"][b][0] for b in range(n_host))
        dev_st, host_st = stats(de_s, B), stats(ho_s, n_host)
        result["cases"].append({"B": B, "frames_mean": sum(lens_all[:B]) / B, "labels_best_mean": sum(len(h[0][0]) - 1 for h in hyps) / B,
                                "device_fused_search": dev_st, "host_loop": host_st, "host_utterances_timed": n_host,
                                "host_over_device": host_st["median_ms_per_utt"] / dev_st["median_ms_per_utt"],
                                "device_max_below_host_min": dev_st["max_ms_per_utt"] < host_st["min_ms_per_utt"],
                                "utterances_with_equal_hypotheses": f"{same}/{n_host}"})

    # the per-frame split, one instrumented pass at the largest B
    B = max(batches)
    row_off = off_all[:B + 1]
    logp, top = logp_all[:row_off[-1]], top_all[:row_off[-1]]
    T = max(lens_all[:B])

    def split_pass():
        t = {"search_launch": 0.0, "record_download": 0.0, "lm_steps": 0.0}
        d_off = torch.tensor(row_off, dtype=torch.int32).to(dev)
        utt = torch.arange(B, dtype=torch.int32).to(dev)
        wt = torch.tensor([[0.3] * B, [0.0] * B], dtype=torch.float64).to(dev)
        st = ops.ctc_beam_lm_init(d_off, utt, W, eos, T)
        lm_pass = cbs._StatefulPass(lm, B * st.slots, V)
        lm_pass(st, int(st.rec_count.item()))
        records = 0
        sync()
        for f in range(T):
            t0 = time.perf_counter()
            ops.ctc_beam_lm_frame(st, f, logp, top, wt[0], wt[1], blank, lm_pass.logp)
            sync()
            t1 = time.perf_counter()
            n = int(st.rec_count.item())
            t2 = time.perf_counter()
            lm_pass(st, n)
            sync()
            t3 = time.perf_counter()
            t["search_launch"] += t1 - t0
            t["record_download"] += t2 - t1
            t["lm_steps"] += t3 - t2
            records += n
        box["split"] = {"B": B, "frames": T, "records_per_frame": records / T,
                        **{name + "_us_per_frame": 1e6 * v / T for name, v in t.items()}}

    split_pass()
    split_pass()
    result["split"] = box["split"]

    # the grid
    G = args.grid_utts
    lm_w, len_w = np.arange(0, 1 + 1e-5, 0.1), np.arange(0, 5 + 1e-5, 1)
    cells = [(float(a), float(b)) for a in lm_w for b in len_w]
    row_off = off_all[:G + 1]
    logp, top = logp_all[:row_off[-1]], top_all[:row_off[-1]]

    def grid():
        box["grid"] = cbs._search_device_lm(logp, top, row_off, W, blank, eos, lm, cells)

    gr_s = timed(grid, args.repeats, sync)
    n_host = min(G, args.host_utts)
    probe = [cells[0], cells[len(cells) // 2], cells[-1]]

    def host_cells():
        box["host_cells"] = []
        for a, b in probe:
            host_loop(n_host, a, b)
            box["host_cells"].append(box["host"])

    hc_s = timed(host_cells, args.repeats, sync)
    scale = (len(cells) / len(probe)) * (G / n_host)
    hyps, _ = box["grid"]
    same = sum(hyps[b][cells.index(c)] == box["host_cells"][i][b][0] for i, c in enumerate(probe) for b in range(n_host))
    grid_st, host_st = stats(gr_s, unit="ms"), stats([s * scale for s in hc_s], unit="ms")
    result["grid"] = {"cells": len(cells), "utterances": G, "searches": len(cells) * G, "device_one_pass": grid_st,
                      "host_scaled": host_st, "host_timed": f"{len(probe)} cells x {n_host} utterances, scaled by {scale:g}",
                      "host_over_device": host_st["median_ms"] / grid_st["median_ms"],
                      "device_max_below_host_min": grid_st["max_ms"] < host_st["min_ms"],
                      "probe_searches_with_equal_hypotheses": f"{same}/{len(probe) * n_host}"}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
