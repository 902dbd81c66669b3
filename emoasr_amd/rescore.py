"""N-best rescoring with a grid search over (lm_weight, len_weight) (asr/rescore/test_rescore_grid.py), with the reference's
function names and argument lists: `score_lm` adds the `score_lm` column of an N-best table (decode.save_results(..., nbest=True)),
`rescore` picks every utterance's best row for one pair of weights and scores it, `grid_search` does so for a whole grid.

The reference aligns the winners with their references again for every cell, in interpreted Python.  Here every (hypothesis,
reference) pair of the table is aligned ONCE (ops.edit_align, csrc/rescore.hip: one wave per pair) and the grid is one launch
(ops.rescore_grid: an arg-max per utterance and three sums per cell).  The score is (score_asr + lm_weight * score_lm) +
len_weight * ylen in f64 with every operation rounded once -- the bits pandas computes -- and ties go to the first row (idxmax),
so the winners, the counts and the WER are the reference's exactly.

    python -m emoasr_amd.rescore NBEST.tsv -ref REF.tsv -lm_conf LM.yaml -lm_ep 40

writes NBEST_{lm_tag}.tsv (the scored table, reused when it exists), NBEST_{lm_tag}.log and NBEST_{lm_tag}_lm{..}_len{..}.tsv (the
best cell's winners).  `-ref` and `-lm_conf` are paths, taken as given; the checkpoint is the reference's
<conf without extension>/checkpoints/model.ep{lm_ep}, or `-lm_ep` itself when that is a file.
"""
import argparse
import logging
import os
import re
import time

import numpy as np
import torch

from . import ops
from .metrics import wer_summary

BATCH_SIZE = 100
EPS = 1e-5


def _ints(s):
    return [int(t) for t in s.split()]


def score_lm(df, model, device, mask_id=None, vocab=None, num_samples=-1):
    """adds df["score_lm"] and returns df: the rows go through model.score in groups of BATCH_SIZE, in table order (with ELECTRA
    the grouping decides which rows meet the one-row sign quirk, see LM.score).  `vocab`: log every hypothesis with its score.
    num_samples > 0 is the reference's --runtime mode: scoring stops at the first row of the num_samples-th utterance (a run of equal
    utt_id), only the full groups before that row are scored, and the ids of the utterances seen so far are returned -- that
    utterance's included, though none of its rows was scored -- with no column added.  A table with fewer utterances is scored whole."""
    rows = [_ints(s) for s in df["token_id"]]
    utts = list(df["utt_id"])
    firsts = [k for k, u in enumerate(utts) if k == 0 or u != utts[k - 1]]
    early = num_samples > 0 and len(firsts) >= num_samples
    n_scored = (firsts[num_samples - 1] // BATCH_SIZE) * BATCH_SIZE if early else len(rows)
    scores = []
    for b0 in range(0, n_scored, BATCH_SIZE):
        group = [torch.tensor(y) for y in rows[b0:b0 + BATCH_SIZE]]
        ys_pad = torch.nn.utils.rnn.pad_sequence(group, batch_first=True).to(device)
        ylens = torch.tensor([len(y) for y in group]).to(device)
        got = model.score(ys_pad, ylens, batch_size=BATCH_SIZE)
        if vocab is not None:
            for y, v in zip(group, got):
                logging.debug(f"{' '.join(vocab.ids2words(y.tolist()))}: {v:.3f}")
        scores.extend(got)
    if early:
        return [utts[k] for k in firsts[:num_samples]]
    df["score_lm"] = scores
    return df


def _words(v):
    return v.split() if isinstance(v, str) else []


class _Table:
    """an N-best table against its references, aligned once: the rows grouped by utterance (a stable sort, so the first row of the
    table is the first row of its group) -- dfref's utterances in its order, then the utterances of df that dfref does not list,
    which get a winner like the others (the reference's groupby keeps them in df_best) but no alignment and zero counts
    (compute_wers_df does not score them) -- one empty hypothesis for every utterance of dfref that has no row, and the word-level
    counts of every row on the device.  An empty hypothesis is the word "<dummy>", as in compute_wer."""

    def __init__(self, df, dfref, device):
        ref_ids = list(dfref["utt_id"])
        utt_of = {u: k for k, u in enumerate(ref_ids)}
        assert len(utt_of) == len(ref_ids), "duplicate utt_id in the reference table"
        vocab = {}
        intern = lambda words: [vocab.setdefault(w, len(vocab)) for w in words]
        refs = [intern(_words(t)) for t in dfref["text"]]
        self.n_ref = sum(len(r) for r in refs)
        U, extra = len(ref_ids), {}
        utt = np.fromiter((utt_of[u] if u in utt_of else extra.setdefault(u, U + len(extra)) for u in df["utt_id"]), np.int64, len(df))
        order = np.argsort(utt, kind="stable")
        missing = np.flatnonzero(np.bincount(utt, minlength=U)[:U] == 0)
        # the table's rows, then one synthetic empty row per missing utterance, sorted by utterance
        all_utt = np.concatenate([utt[order], missing])
        src = np.concatenate([order, np.full(len(missing), -1)])
        perm = np.argsort(all_utt, kind="stable")
        self.src = src[perm]                                  # table row (position in df) of each device row, -1: synthetic
        row_utt = all_utt[perm]
        scored = row_utt < U
        text = list(df["text"])
        hyps = [intern((_words(text[k]) if k >= 0 else []) or ["<dummy>"]) for k in self.src[scored]]
        counts = np.zeros((len(row_utt), 4), np.int32)
        counts[scored] = ops.edit_align(hyps, refs, ref_idx=row_utt[scored], device=device)["counts"]
        score_asr = df["score_asr"].to_numpy(np.float64)
        score_lm_ = df["score_lm"].to_numpy(np.float64)
        ylen = df["token_id"].apply(lambda s: len(s.split())).to_numpy(np.int64)
        pick = lambda a: np.append(a, 0)[self.src]              # (src -1, a synthetic row: the appended 0)
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
        self.counts = dev(counts, np.int32)
        self.score_asr, self.score_lm = dev(pick(score_asr), np.float64), dev(pick(score_lm_), np.float64)
        self.ylen = dev(pick(ylen), np.int32)
        self.utt_off = dev(np.concatenate([[0], np.cumsum(np.bincount(row_utt, minlength=U + len(extra)))]), np.int32)
        self.device = device

    def grid(self, lm_weights, len_weights):
        """-> (best [G, U] device-row index, totals [G, 3] = S, I, D) as host arrays"""
        w = lambda a: torch.tensor(np.asarray(a, np.float64).reshape(-1), dtype=torch.float64, device=self.device)
        best, totals = ops.rescore_grid(self.score_asr, self.score_lm, self.ylen, self.utt_off, self.counts, w(lm_weights),
                                        w(len_weights))
        return best.cpu().numpy(), totals.cpu().numpy()


def _device_of(device):
    return torch.device("cuda") if device is None else torch.device(device)


def _df_best(df, src_rows):
    rows = np.sort(src_rows[src_rows >= 0])
    df_best = df.iloc[rows]
    # (the reference's groupby lists the winners by sorted utt_id)
    df_best = df_best.sort_values("utt_id", kind="stable")
    return df_best[["utt_id", "text", "token_id", "score_asr"]]


def grid_search(df, dfref, lm_weights, len_weights, device=None):
    """-> (table, best): table[a][b] = (wer, wer_dict) of rescore(df, dfref, lm_weights[a], len_weights[b]); best = dict(lm_weight,
    len_weight, wer, wer_dict, df_best) of the first cell, lm_weights outer, whose WER is strictly below every earlier one's, starting
    from 100 as the reference's loop does (no cell below 100: weights 0, wer 100, df_best None)."""
    lm_weights, len_weights = [np.float64(v) for v in lm_weights], [np.float64(v) for v in len_weights]
    table = _Table(df, dfref, _device_of(device))
    best_rows, totals = table.grid(lm_weights, len_weights)
    G2 = len(len_weights)
    out = [[None] * G2 for _ in lm_weights]
    best = {"lm_weight": 0, "len_weight": 0, "wer": 100, "wer_dict": None, "df_best": None}
    arg = None
    for a, wl in enumerate(lm_weights):
        for b, wn in enumerate(len_weights):
            s, i, d = (int(v) for v in totals[a * G2 + b])
            wer = ((s + i + d) / table.n_ref) * 100      # (the reference's order of operations, metrics.py:166)
            wer_dict = {"n_sub": s, "n_ins": i, "n_del": d, "n_ref": table.n_ref, "wer": wer}
            out[a][b] = (wer, wer_dict)
            if wer < best["wer"]:
                best.update(lm_weight=wl, len_weight=wn, wer=wer, wer_dict=wer_dict)
                arg = a * G2 + b
    if arg is not None:
        best["df_best"] = _df_best(df, table.src[best_rows[arg]])
    return out, best


def rescore(df, dfref, lm_weight, len_weight, device=None):
    """-> (wer, wer_dict, df_best): grid_search with one cell.  As in the reference, df gains the columns ylen and score."""
    lm_weight, len_weight = np.float64(lm_weight), np.float64(len_weight)
    df["ylen"] = df["token_id"].apply(lambda s: len(s.split()))
    df["score"] = df["score_asr"] + lm_weight * df["score_lm"] + len_weight * df["ylen"]
    table = _Table(df, dfref, _device_of(device))
    best_rows, totals = table.grid([lm_weight], [len_weight])
    s, i, d = (int(v) for v in totals[0])
    wer = ((s + i + d) / table.n_ref) * 100      # (the reference's order of operations, metrics.py:166)
    return wer, {"n_sub": s, "n_ins": i, "n_del": d, "n_ref": table.n_ref, "wer": wer}, _df_best(df, table.src[best_rows[0]])


def load_config(path):
    import yaml
    from types import SimpleNamespace
    with open(path, encoding="utf-8") as f:
        return SimpleNamespace(**yaml.safe_load(f))


def model_path(lm_conf, lm_ep):
    return lm_ep if os.path.isfile(str(lm_ep)) else os.path.join(os.path.splitext(lm_conf)[0], "checkpoints", f"model.ep{lm_ep}")


# the reference's command line: (flag, type or None for a switch, default or REQUIRED)
REQUIRED = object()
ARGUMENTS = [("tsv_path", str, REQUIRED), ("-ref", str, REQUIRED), ("-lm_conf", str, REQUIRED), ("-lm_ep", str, REQUIRED),
             ("--lm_tag", str, None), ("--cpu", None, False), ("--debug", None, False), ("--runtime", None, False),
             ("--runtime_num_samples", int, 20), ("--runtime_num_repeats", int, 5), ("--wavtime_factor", float, 1000),
             ("--lm_min", float, 0), ("--lm_max", float, 1), ("--lm_step", float, 0.1),
             ("--len_min", float, 0), ("--len_max", float, 5), ("--len_step", float, 1)]


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m emoasr_amd.rescore", description=__doc__.split("\n\n")[0])
    for flag, kind, default in ARGUMENTS:
        if kind is None:
            parser.add_argument(flag, action="store_true")
        elif not flag.startswith("-"):
            parser.add_argument(flag, type=kind)
        elif default is REQUIRED:
            parser.add_argument(flag, type=kind, required=True)
        else:
            parser.add_argument(flag, type=kind, default=default)
    return parser


def _wav_seconds(utt_id, factor):
    """an utterance id ends in ..._<start>_<end> (or -<start>-<end>), in 1 / factor seconds"""
    start, end = re.split("_|-", utt_id)[-2:]
    return (int(end) - int(start)) / factor


def runtime_mode(df, lm, device, mask_id, args):
    """--runtime: one row per model.score call over the first utterances, `runtime_num_repeats` times; logs time and real-time factor"""
    global BATCH_SIZE
    BATCH_SIZE = 1
    runtimes, rtfs = [], []
    for j in range(args.runtime_num_repeats):
        torch.cuda.synchronize()
        t0 = time.time()
        utt_ids = score_lm(df, lm, device, mask_id=mask_id, num_samples=args.runtime_num_samples)
        torch.cuda.synchronize()
        runtime = time.time() - t0
        wavtime = sum(_wav_seconds(u, args.wavtime_factor) for u in utt_ids)
        logging.info(f"Run {(j+1):d} runtime: {runtime:.5f}sec / utt, wavtime: {wavtime:.5f}sec | RTF: {(runtime / wavtime):.5f}")
        runtimes.append(runtime)
        rtfs.append(runtime / wavtime)
    logging.info(f"Averaged runtime {np.mean(runtimes):.5f}sec, RTF {np.mean(rtfs):.5f} on {device.type}")


def main(args):
    import pandas as pd
    from .datasets import Vocab
    from .modeling.lm import LM
    if args.cpu:
        raise SystemExit("emoasr_amd.rescore: --cpu is the reference's host mode; the LM and the alignment here run on the device only")
    device = torch.device("cuda")
    lm_params = load_config(args.lm_conf)
    lm_tag = args.lm_tag or lm_params.lm_type
    scored_tsv_path = args.tsv_path.replace(".tsv", f"_{lm_tag}.tsv")
    to_console = args.debug or args.runtime
    logging.basicConfig(filename=None if to_console else args.tsv_path.replace(".tsv", f"_{lm_tag}.log"),
                        level=logging.DEBUG if to_console else logging.INFO,
                        format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    lm_path = model_path(args.lm_conf, args.lm_ep)
    lm = LM(lm_params, phase="test")
    lm.load_state_dict(torch.load(lm_path, map_location="cpu"))
    lm.to(device).eval()
    logging.info(f"LM: {lm_path}")
    mask_id = getattr(lm_params, "mask_id", None)
    df, dfref = pd.read_table(args.tsv_path).dropna(), pd.read_table(args.ref)
    if args.runtime:
        return runtime_mode(df, lm, device, mask_id, args)

    if os.path.exists(scored_tsv_path):
        logging.info(f"load score_lm: {scored_tsv_path}")
        df = pd.read_table(scored_tsv_path)
    else:
        df = score_lm(df, lm, device, mask_id=mask_id, vocab=Vocab(lm_params.vocab_path) if args.debug else None)
        df.to_csv(scored_tsv_path, sep="\t", index=False)

    lm_weights = np.arange(args.lm_min, args.lm_max + EPS, args.lm_step)
    len_weights = np.arange(args.len_min, args.len_max + EPS, args.len_step)
    table, best = grid_search(df, dfref, lm_weights, len_weights, device=device)
    for a, lm_weight in enumerate(lm_weights):
        for b, len_weight in enumerate(len_weights):
            logging.info(f"lm_weight: {lm_weight:.3f} len_weight: {len_weight:.3f} - {wer_summary(*table[a][b])}")
    logging.info(f"best lm_weight: {best['lm_weight']:.3f} len_weight: {best['len_weight']:.3f}")
    if best["df_best"] is not None:
        best["df_best"].to_csv(scored_tsv_path.replace(".tsv", f"_lm{best['lm_weight']:.2f}_len{best['len_weight']:.2f}.tsv"),
                               sep="\t", index=False)
    logging.info(f"best WER: {best['wer']:.3f}")


if __name__ == "__main__":
    main(build_parser().parse_args())
