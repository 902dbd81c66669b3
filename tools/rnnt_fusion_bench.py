"""Measure RNN-LM shallow fusion in the transducer beam search: a measurement, not a gate.

    python tools/rnnt_fusion_bench.py [--beams 4,10] [--batches 1,16,64] [--repeats 5] [--host-utts 2] [--grid-cells 6] [--out FILE]

The L4-sized transducer of bench.py (V = 1000, H = 512, J = 512, two LSTM layers, bf16) and a 2-layer RNN LM (V = 1000, embedding
512, hidden 512, bf16), both with seeded random weights, on seeded random encoder outputs for utterances of 180 .. 300 encoder
frames.  For each beam width and batch size B, in one process:

  fused device   engine.rnnt_beam_search_batch(..., lm=, lm_weights=[0.3], len_weights=[0]) on the B utterances
  fused host     engine._rnnt_beam_search_chain with the same LM and weight (the host form: lm.predict per round, the
                 bookkeeping in Python) on the first --host-utts of them, one after the other
  plain device   engine.rnnt_beam_search_batch without an LM on the B utterances (the cost of fusion per frame comes from the two)

and at B = 16 the default 11 x 6 grid (lm_weight 0 .. 1 by 0.1, len_weight 0 .. 5) in ONE call against batched single-cell calls:
--grid-cells of the 66 cells are timed, spread over the lm_weights, and their mean is scaled to 66 (the JSON says so).

Every timing is a host clock around work that ends in a device synchronise, after one warm-up run of the same shape; the forms
alternate repeat by repeat; the median of --repeats is reported per utterance, minimum and maximum next to it.  Prints one JSON
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
    ap.add_argument("--beams", type=str, default="4,10")
    ap.add_argument("--batches", type=str, default="1,16,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-utts", type=int, default=2)
    ap.add_argument("--grid-cells", type=int, default=6)
    ap.add_argument("--grid-batch", type=int, default=16)
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    import bench
    from emoasr_amd.fusion_grid import weight_lists
    from emoasr_amd.hostenv import respect_cpu_quota
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.lm import LM
    if not torch.cuda.is_available():
        raise SystemExit("rnnt_fusion_bench: no GPU (there is nothing to measure on the host alone)")
    respect_cpu_quota()
    dev, sync = torch.device("cuda"), torch.cuda.synchronize
    torch.manual_seed(2)
    model = ASR(SimpleNamespace(**bench.L4), compute_dtype=torch.bfloat16).to(dev).eval()
    V = bench.L4["vocab_size"]
    lm = LM(SimpleNamespace(lm_type="rnn", vocab_size=V, embedding_size=512, hidden_size=512, num_layers=2, dropout_rate=0.0,
                            tie_weights=False), compute_dtype=torch.bfloat16).to(dev).eval()
    eng = model.engine()
    eng.ensure_bound()
    assert eng.rnnt_beam_lm_why_not(lm) is None, eng.rnnt_beam_lm_why_not(lm)
    blank, eos = model.decoder.blank_id, model.decoder.eos_id
    batches = [int(b) for b in args.batches.split(",")]
    nmax = max(batches + [args.grid_batch])
    lens_all = [int(n) for n in np.random.default_rng(0).integers(180, 301, nmax)]
    g = torch.Generator().manual_seed(0)
    eouts_all = torch.randn(nmax, 300, bench.L4["enc_hidden_size"], generator=g).to(dev, torch.bfloat16)
    mu = args.lm_weight
    result = {"device": torch.cuda.get_device_name(0), "model": "L4 (V=1000, H=512, J=512, 2 layers, bf16)",
              "lm": "RNN LM (V=1000, E=512, H=512, 2 layers, bf16)", "frames": "180..300", "lm_weight": mu, "cases": [], "grid": []}
    with torch.no_grad():
        for W in [int(w) for w in args.beams.split(",")]:
            for B in batches:
                lens, eouts = lens_all[:B], eouts_all[:B]
                nh = min(B, args.host_utts)
                box = {}
                forms = {
                    "fused": lambda: box.__setitem__("fused", eng.rnnt_beam_search_batch(eouts, lens, W, blank, eos, lm=lm,
                                                                                         lm_weights=[mu], len_weights=[0.0])),
                    "host": lambda: box.__setitem__("host", [eng._rnnt_beam_search_chain(eouts[b:b + 1, :lens[b]], W, blank, eos, 3, True,
                                                                                        lm, mu, 0.0) for b in range(nh)]),
                    "plain": lambda: box.__setitem__("plain", eng.rnnt_beam_search_batch(eouts, lens, W, blank, eos)),
                }
                s = alternate(forms, args.repeats, sync)
                fh = [h[0] for h in box["fused"][0]]
                same = sum(int(fh[b][0] == box["host"][b][0][0]) for b in range(nh))
                moved = sum(int(fh[b][0] != box["plain"][0][b][0]) for b in range(B))
                fm, hm, pm = (statistics.median(s[k]) / n for k, n in (("fused", B), ("host", nh), ("plain", B)))
                frames = sum(lens) / B
                print(f"W={W} B={B} fused {1e3 * fm:.2f} host {1e3 * hm:.2f} plain {1e3 * pm:.2f} ms/utt", file=sys.stderr, flush=True)
                result["cases"].append({"W": W, "B": B, "frames_mean": frames, "fused_device": per_utt(s["fused"], B),
                                        "fused_host": per_utt(s["host"], nh), "host_utts": nh, "plain_device": per_utt(s["plain"], B),
                                        "host_over_fused": hm / fm, "fused_over_plain": fm / pm,
                                        "fusion_us_per_frame": 1e6 * (fm - pm) / frames, "best_hyps_equal_host": f"{same}/{nh}",
                                        "best_hyps_moved_by_fusion": f"{moved}/{B}"})
            # the grid at --grid-batch utterances: one call against single-cell calls (a subset, scaled)
            B = args.grid_batch
            lens, eouts = lens_all[:B], eouts_all[:B]
            lm_ws, len_ws = weight_lists(0, 1, 0.1, 0, 5, 1)
            cells = [(float(a), float(b)) for a in lm_ws for b in len_ws]
            pick = [cells[i] for i in np.linspace(0, len(cells) - 1, args.grid_cells).round().astype(int)]
            forms = {
                "grid": lambda: eng.rnnt_beam_search_batch(eouts, lens, W, blank, eos, lm=lm, lm_weights=list(lm_ws), len_weights=list(len_ws)),
                "cells": lambda: [eng.rnnt_beam_search_batch(eouts, lens, W, blank, eos, lm=lm, lm_weights=[a], len_weights=[b])
                                  for a, b in pick],
            }
            s = alternate(forms, max(1, min(args.repeats, 3)), sync)
            gm, cm = statistics.median(s["grid"]), statistics.median(s["cells"]) / len(pick) * len(cells)
            print(f"W={W} grid {gm:.2f} s, {len(cells)} single-cell calls {cm:.2f} s (scaled from {len(pick)})", file=sys.stderr, flush=True)
            result["grid"].append({"W": W, "B": B, "cells": len(cells), "grid_call_s": {"median": gm, "min": min(s["grid"]), "max": max(s["grid"])},
                                   "single_cell_calls_s_scaled": cm, "cells_timed": len(pick), "scaled_from_subset": True,
                                   "cells_over_grid": cm / gm, "n": len(s["grid"])})
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
