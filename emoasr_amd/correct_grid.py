"""CTC error correction over a grid of (mask_th, lm_weight) cells in ONE pass over the data (asr/test_asr_correct.py, once per cell).

The reference corrects the test set once per cell; every such run repeats the encoder pass, and every lm_weight repeats the LM pass.
Neither depends on the weight, and the encoder pass does not depend on the threshold: here every batch is encoded once and
correct.correct_batch corrects it for all cells -- one LM pass per threshold that masks something, one fuse launch for all weights.

    results = correct_grid(model, lm, dataloader, vocab, vocab_size, device, blank_id, mask_id, mask_ths, lm_weights)
    python -m emoasr_amd.correct_grid -conf asr.yaml -ep 40 -lm_conf lm.yaml -lm_ep 20 --lm_weight 0,0.5,1 --mask_th 0.8,0.9

results = [(mask_th, lm_weight, rows, wer, wer_dict, num_masked, num_tokens), ...], mask_th outer; rows = [utt_id, token_id, text,
reftext] as correct.test returns them.  The command writes one result TSV per cell under the reference's file name
(result_{data_tag}_{lm_tag}_corr{w}_maskth{th}_ep{ep}.tsv, its WER comment on top) and one summary TSV over the cells.  LM kinds:
"bert" and "pbert"; "pctc" is the cascade and has no grid (one cell, whatever the lists say).
"""
import argparse
import logging
import os

import torch

from . import correct
from .decode import ints2str
from .metrics import compute_wers_cells, wer_summary

GRID_BATCH = 16      # utterances per correct_batch call of the command-line tool


def float_list(text):
    """"0,0.5,1" -> [0.0, 0.5, 1.0] (a single number is a one-entry list)"""
    vals = [float(v) for v in str(text).split(",") if v.strip()]
    if not vals:
        raise argparse.ArgumentTypeError(f"no number in {text!r}")
    return vals


def correct_grid(model, lm, dataloader, vocab, vocab_size, device, blank_id, mask_id, mask_ths, lm_weights, pad_id=0,
                 cascade_ctc=False):
    """-> [(mask_th, lm_weight, rows, wer, wer_dict, num_masked, num_tokens)] over mask_ths x lm_weights (mask_ths outer).  One pass
    over the loader; every distinct (utterance, corrected text) pair is aligned once (metrics.compute_wers_cells)."""
    ths, ws = correct._grid_axis(mask_ths), correct._grid_axis(lm_weights)
    if cascade_ctc:
        ths, ws = ths[:1], ws[:1]
    cells = [(th, w) for th in ths for w in ws]
    rows_of = [[] for _ in cells]
    masked, tokens = [0] * len(cells), [0] * len(cells)
    for data in dataloader:
        out = correct.correct_batch(model, lm, data, blank_id, mask_id, ths, ws, device, vocab_size, pad_id=pad_id,
                                    cascade_ctc=cascade_ctc)
        for c in range(len(cells)):
            for utt_id, hyp, hyp_cor, reftext, num_masked, num_tokens in out[c // len(ws)][c % len(ws)]:
                masked[c] += num_masked
                tokens[c] += num_tokens
                if len(hyp) < 1:
                    logging.warning(f"cannot decode {utt_id}")
                    rows_of[c].append([utt_id, None, "", reftext])
                else:
                    rows_of[c].append([utt_id, ints2str(hyp_cor), vocab.ids2text(hyp_cor), reftext])
    refs = [r[3].split() for r in rows_of[0]]
    wers = compute_wers_cells([[r[2].split() for r in rows] for rows in rows_of], refs, device=device)
    return [(th, w, rows_of[c], wers[c][0], wers[c][1], masked[c], tokens[c]) for c, (th, w) in enumerate(cells)]


def write_results(results, results_dir, data_tag, lm_tag, ep):
    """one TSV per cell (utt_id, token_id, text, reftext; '# WER ...' and '#' on top, as the reference's insert_comment leaves it)
    and summary_{data_tag}_{lm_tag}_ep{ep}.tsv -> the summary's path"""
    import pandas as pd
    os.makedirs(results_dir, exist_ok=True)
    summary = []
    for th, w, rows, wer, wd, num_masked, num_tokens in results:
        path = os.path.join(results_dir, f"result_{data_tag}_{lm_tag}_corr{w}_maskth{th}_ep{ep}.tsv")
        info = wer_summary(wer, wd)
        with open(path, "w", encoding="utf-8") as f:
            f.write(f"# {info}\n#\n")
            pd.DataFrame(rows, columns=["utt_id", "token_id", "text", "reftext"]).to_csv(f, sep="\t", index=False)
        logging.info(f"mask_th: {th} lm_weight: {w} - {info} masked: {num_masked:d} / {num_tokens:d} -> {path}")
        summary.append([th, w, wer, wd["n_sub"], wd["n_ins"], wd["n_del"], wd["n_ref"], num_masked, num_tokens])
    path = os.path.join(results_dir, f"summary_{data_tag}_{lm_tag}_ep{ep}.tsv")
    pd.DataFrame(summary, columns=["mask_th", "lm_weight", "wer", "n_sub", "n_ins", "n_del", "n_ref", "num_masked",
                                   "num_tokens"]).to_csv(path, sep="\t", index=False)
    return path


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m emoasr_amd.correct_grid", description=__doc__.split("\n\n")[0])
    parser.add_argument("-conf", type=str, required=True)
    parser.add_argument("-ep", type=str, required=True)
    parser.add_argument("-lm_conf", type=str, required=True)
    parser.add_argument("-lm_ep", type=str, required=True)
    parser.add_argument("--lm_weight", type=float_list, default=[1.0], help="comma-separated list")
    parser.add_argument("--mask_th", type=float_list, default=[0.9], help="comma-separated list")
    parser.add_argument("--cpu", action="store_true")
    parser.add_argument("--data", type=str, default=None)
    parser.add_argument("--data_tag", type=str, default="test")
    parser.add_argument("--lm_tag", type=str, default=None)
    parser.add_argument("--debug", action="store_true")
    parser.add_argument("--runtime", action="store_true")
    parser.add_argument("--runtime_num_samples", type=int, default=20)
    parser.add_argument("--runtime_num_repeats", type=int, default=5)
    parser.add_argument("--wavtime_factor", type=float, default=1000)
    return parser


def _loader(dataset, n):
    for i in range(0, len(dataset), n):
        yield dataset.collate_fn([dataset[j] for j in range(i, min(i + n, len(dataset)))])


def main(args):
    from .datasets import ASRDataset, Vocab
    from .modeling.asr import ASR
    from .modeling.lm import LM
    from .modeling.p2w import P2W
    from .rescore import load_config, model_path
    if args.cpu:
        raise SystemExit("emoasr_amd.correct_grid: --cpu is not available (the kernels run on the device only)")
    if args.runtime:
        raise NotImplementedError("emoasr_amd.correct_grid: the --runtime RTF protocol is not built")
    params = load_config(args.conf)
    assert params.decoder_type == "ctc"
    lm_params = load_config(args.lm_conf)
    if lm_params.lm_type not in ("bert", "pbert", "pctc"):
        raise NotImplementedError(f"emoasr_amd.correct_grid: lm_type {lm_params.lm_type!r}; 'bert', 'pbert' or 'pctc' (the cascade)")
    device = torch.device("cuda")
    logging.basicConfig(format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s", level=logging.INFO)
    model = ASR(params, phase="test")
    model.load_state_dict(torch.load(model_path(args.conf, args.ep), map_location="cpu"))
    model.to(device).eval()
    lm = (LM if lm_params.lm_type == "bert" else P2W)(lm_params, phase="test")
    lm.load_state_dict(torch.load(model_path(args.lm_conf, args.lm_ep), map_location="cpu"))
    lm.to(device).eval()
    data_path = args.data or params.test_path
    data_tag = args.data if args.data_tag == "test" and data_path != args.data and args.data else args.data_tag
    data_tag = os.path.splitext(os.path.basename(data_tag))[0]
    dataset = ASRDataset(params, data_path, phase="test")
    results = correct_grid(model, lm, _loader(dataset, GRID_BATCH), Vocab(params.vocab_path), params.vocab_size, device,
                           params.blank_id, lm_params.mask_id, args.mask_th, args.lm_weight,
                           cascade_ctc=lm_params.lm_type == "pctc")
    lm_tag = lm_params.lm_type if args.lm_tag is None else args.lm_tag
    path = write_results(results, os.path.join(os.path.splitext(args.conf)[0], "results"), data_tag, lm_tag, args.ep)
    logging.info(f"summary: {path}")
    return results


if __name__ == "__main__":
    main(build_parser().parse_args())
