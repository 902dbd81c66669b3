"""Restatements of the label fold of align_hyps and of the rescoring grid (emoasr_amd/rescore.py, emoasr_amd/align_hyps.py,
csrc/rescore.hip), written from behaviour: plain python over lists and float64 scalars.  Shared by tests/test_rescore_cpu.py (held
to the reference's outputs there) and tests/test_rescore_gpu.py.  The alignment itself is emoasr_amd.metrics.compute_wer."""
import numpy as np


def fold_labels(ops, mode):
    """ops: sequence of C / S / I / D -> one label per non-D op.  "SI": the ops without the deletions.  "SID": a deletion with no
    label before it, or after a label other than C, turns the next C into D; a deletion after a C changes nothing (the reference
    compares there where it means to assign)."""
    assert mode in ("SI", "SID")
    out, flag = [], False
    for e in ops:
        if e == "D":
            if mode == "SID" and not (out and out[-1] == "C"):
                flag = True
        else:
            out.append("D" if flag and e == "C" else e)
            flag = False
    return out


def grid_ref(score_asr, score_lm, ylen, utt_off, counts, lm_w, len_w):
    """-> (best [G1*G2, U], totals [G1*G2, 3]): per cell and utterance the first row with the largest
    (score_asr + lm_w * score_lm) + len_w * ylen, each operation a float64 operation of its own (numpy scalars: no fused
    multiply-add), -1 for an utterance without rows; the winners' counts[:, :3] summed"""
    U = len(utt_off) - 1
    best = np.full((len(lm_w) * len(len_w), U), -1, np.int64)
    totals = np.zeros((len(lm_w) * len(len_w), 3), np.int64)
    for a, wl in enumerate(lm_w):
        for b, wn in enumerate(len_w):
            g = a * len(len_w) + b
            for u in range(U):
                top = None
                for k in range(int(utt_off[u]), int(utt_off[u + 1])):
                    s = (np.float64(score_asr[k]) + np.float64(wl) * np.float64(score_lm[k])) + np.float64(wn) * np.float64(ylen[k])
                    if top is None or s > top:
                        top, best[g, u] = s, k
                if top is not None:
                    totals[g] += np.asarray(counts[best[g, u]][:3], np.int64)
    return best, totals
