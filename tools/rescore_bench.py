"""Measure N-best rescoring and error-label alignment on the device against the host code (a measurement, not a gate).

    python tools/rescore_bench.py [--utts 2620] [--nbest 10] [--ref-len 20] [--pairs 2000] [--repeats 5] [--host-cells 3] [--out FILE]

  grid        a synthetic N-best of a test set's size (2 620 utterances x 10 hypotheses, 20-word references, the default 11 x 6
              grid of test_rescore_grid): emoasr_amd.rescore.grid_search end to end (interning the words, the upload, one
              emoasr_edit_align call, one emoasr_rescore_grid call, the download) against the same grid done the reference's way on
              the host: per cell the pandas score / groupby / idxmax and metrics.compute_wers_df over the winners.  The host cell
              costs seconds, so `--host-cells` cells are timed (each one sample) and the grid is their median times the cell count.
  alignment   emoasr_amd.align_hyps.alignment over `--pairs` hypotheses of 256 tokens against 256-token references (align_hyps'
              default len_max) against the host loop (metrics.compute_wer + the label fold) -- timed on `--host-pairs` pairs and
              scaled per pair.

Every device timing is a host clock around work that ends in a device synchronise, after one warm-up run, repeated `--repeats`
times: median, minimum and maximum are reported.  The device results are compared with the host's on what the host computed.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def mutate(rng, ref, vocab, rate):
    hyp = []
    for t in ref:
        x = rng.random()
        if x < rate:
            continue
        hyp.append(int(rng.integers(0, vocab)) if x < 2 * rate else t)
        if rng.random() < rate:
            hyp.append(int(rng.integers(0, vocab)))
    return hyp or [int(rng.integers(0, vocab))]


def nbest_tables(rng, utts, nbest, ref_len, vocab=1000):
    import pandas as pd
    text = lambda seq: " ".join(f"w{k}" for k in seq)
    ids = lambda seq: " ".join(str(k + 3) for k in seq)
    ref_rows, rows = [], []
    for u in range(utts):
        ref = rng.integers(0, vocab, ref_len).tolist()
        ref_rows.append((f"utt-{u:05d}", ids(ref), text(ref)))
        for _ in range(nbest):
            hyp = mutate(rng, ref, vocab, 0.08)
            rows.append((f"utt-{u:05d}", float(-rng.random() * 20), float(-rng.random() * 40), ids(hyp), text(hyp), text(ref)))
    return (pd.DataFrame(rows, columns=["utt_id", "score_asr", "score_lm", "token_id", "text", "reftext"]),
            pd.DataFrame(ref_rows, columns=["utt_id", "token_id", "text"]))


def stats(samples):
    return {"median_s": statistics.median(samples), "min_s": min(samples), "max_s": max(samples), "n": len(samples)}


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


def host_cell(df, dfref, lm_weight, len_weight):
    """test_rescore_grid.rescore with the host metrics"""
    from emoasr_amd.metrics import compute_wers_df
    df["ylen"] = df["token_id"].apply(lambda s: len(s.split()))
    df["score"] = df["score_asr"] + lm_weight * df["score_lm"] + len_weight * df["ylen"]
    df_best = df.loc[df.groupby("utt_id")["score"].idxmax(), :]
    return compute_wers_df(df_best[["utt_id", "text", "token_id", "score_asr"]], dfref)


def host_alignment(dfhyp, dfref, align_type):
    """align_hyps.alignment's loop with the host metrics"""
    from emoasr_amd.metrics import compute_wer
    id2ref = {r.utt_id: r.token_id.split() for r in dfref.itertuples()}
    out = []
    for row in dfhyp.itertuples():
        ops = compute_wer(row.token_id.split(), id2ref[row.utt_id])[1]["error_list"]
        labels, flag = [], False
        for e in ops:
            if e == "D":
                if align_type == "SID" and not (labels and labels[-1] == "C"):
                    flag = True
            else:
                labels.append("D" if flag and e == "C" else e)
                flag = False
        out.append(" ".join(labels))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2620)
    ap.add_argument("--nbest", type=int, default=10)
    ap.add_argument("--ref-len", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--host-pairs", type=int, default=5)
    ap.add_argument("--host-cells", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    from emoasr_amd import align_hyps, rescore
    if not torch.cuda.is_available():
        raise SystemExit("rescore_bench: no GPU (there is nothing to measure on the host alone)")
    dev, sync = torch.device("cuda"), torch.cuda.synchronize
    rng = np.random.default_rng(0)
    result = {"device": torch.cuda.get_device_name(0)}

    # ---- grid
    df, dfref = nbest_tables(rng, args.utts, args.nbest, args.ref_len)
    lm_w, len_w = np.arange(0, 1 + rescore.EPS, 0.1), np.arange(0, 5 + rescore.EPS, 1)
    cells = len(lm_w) * len(len_w)
    box = {}

    def run_grid():
        box["table"], box["best"] = rescore.grid_search(df, dfref, lm_w, len_w, device=dev)

    dev_s = timed(run_grid, args.repeats, sync)
    table = rescore._Table(df, dfref, dev)
    kern_s = timed(lambda: table.grid(lm_w, len_w), args.repeats, sync)
    picks = [(0, 0), (len(lm_w) // 2, len(len_w) // 2), (len(lm_w) - 1, len(len_w) - 1)][: args.host_cells]
    host_s = []
    for a, b in picks:
        work = df.copy()            # (host_cell adds columns; the copy is not part of the cell)
        t0 = time.perf_counter()
        _, hw = host_cell(work, dfref, lm_w[a], len_w[b])
        host_s.append(time.perf_counter() - t0)
        dw = box["table"][a][b][1]
        assert all(dw[k] == hw[k] for k in ("n_sub", "n_ins", "n_del", "n_ref")), (a, b, dw, hw)
    host_grid = statistics.median(host_s) * cells
    result["grid"] = {"utts": args.utts, "rows": len(df), "cells": cells, "device_grid_search": stats(dev_s),
                      "device_grid_launch_only": stats(kern_s), "host_cell": stats(host_s), "host_grid_s_scaled": host_grid,
                      "speedup": host_grid / statistics.median(dev_s), "best": [float(box["best"]["lm_weight"]),
                                                                                 float(box["best"]["len_weight"]), box["best"]["wer"]]}

    # ---- alignment at 256-token pairs
    dfh, dfr = nbest_tables(rng, args.pairs, 1, 256, vocab=40)
    dfh = dfh[dfh["token_id"].apply(lambda s: len(s.split()) <= 256)].reset_index(drop=True)
    box2 = {}

    def run_align():
        box2["df"] = align_hyps.alignment(dfh, dfr, align_type="SID", device=dev)

    adev_s = timed(run_align, args.repeats, sync)
    t0 = time.perf_counter()
    want = host_alignment(dfh.iloc[: args.host_pairs], dfr, "SID")
    host_pair = (time.perf_counter() - t0) / args.host_pairs
    assert box2["df"]["error_label"].tolist()[: args.host_pairs] == want
    result["alignment"] = {"pairs": len(dfh), "tokens_per_side": 256, "device_alignment": stats(adev_s),
                           "host_s_per_pair": host_pair, "host_pairs_timed": args.host_pairs,
                           "host_s_scaled": host_pair * len(dfh), "speedup": host_pair * len(dfh) / statistics.median(adev_s)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
