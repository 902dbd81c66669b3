"""Align N-best hypotheses with their references to train `electra-disc` / `pelectra-disc` (asr/rescore/align_hyps.py): the
`error_label` column LMDataset reads, one of C / S / I / D per hypothesis token.

Every (hypothesis, reference) pair of the table goes through ONE ops.edit_align call (csrc/rescore.hip: one wave per pair, the
reference's backtrace preference and its label fold, "SID" quirk included -- see the kernel's header); the reference runs
compute_wer per row in interpreted Python.

    python -m emoasr_amd.align_hyps NBEST.tsv -ref REF.tsv [--align_type SID]      ->  NBEST_SIDalign.tsv
"""
import argparse

import torch

from . import ops


def _ints(s):
    return [int(t) for t in s.split()]


def alignment(dfhyp, dfref, align_type="SID", len_min=1, len_max=256, device=None):
    """-> DataFrame(utt_id, score_asr, token_id, text, reftext, error_label) over the rows of dfhyp whose token count lies in
    [len_min, len_max], in table order.  A hypothesis of no tokens has no label row and is skipped whatever len_min says (the
    reference's assert fails on it)."""
    import pandas as pd
    assert align_type in ("SI", "SID"), align_type
    utt_of, refs = {}, []
    for row in dfref.itertuples():
        if row.utt_id not in utt_of:
            refs.append(None)
        utt_of.setdefault(row.utt_id, len(refs) - 1)
        refs[utt_of[row.utt_id]] = _ints(row.token_id)      # (a repeated utt_id: the last row wins, as in the reference's dict)
    rows, hyps, ref_idx = [], [], []
    for row in dfhyp.itertuples():
        hyp = _ints(row.token_id)
        r = utt_of[row.utt_id]
        if len(hyp) < len_min or len(hyp) > len_max or not hyp:
            continue
        rows.append(row)
        hyps.append(hyp)
        ref_idx.append(r)
    labels = []
    if rows:
        device = torch.device("cuda") if device is None else torch.device(device)
        labels = ops.edit_align(hyps, refs, ref_idx=ref_idx, device=device, label_mode=align_type)["labels"]
    outs = [(row.utt_id, row.score_asr, row.token_id, row.text, row.reftext, " ".join(lab)) for row, lab in zip(rows, labels)]
    return pd.DataFrame(outs, columns=["utt_id", "score_asr", "token_id", "text", "reftext", "error_label"])


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m emoasr_amd.align_hyps")
    parser.add_argument("tsv_path", type=str)
    parser.add_argument("-ref", type=str, required=True)
    parser.add_argument("--align_type", choices=["SI", "SID"], default="SID")
    parser.add_argument("--len_min", type=int, default=1)
    parser.add_argument("--len_max", type=int, default=256)
    return parser


def main(args):
    import pandas as pd
    dfhyp = pd.read_table(args.tsv_path).dropna()
    dfref = pd.read_table(args.ref)
    df = alignment(dfhyp, dfref, args.align_type, len_min=args.len_min, len_max=args.len_max)
    df.to_csv(args.tsv_path.replace(".tsv", f"_{args.align_type}align.tsv"), sep="\t", index=False)


if __name__ == "__main__":
    main(build_parser().parse_args())
