"""Restatements of the correction grid's kernels (csrc/correct.hip: emoasr_correct_mask_grid, emoasr_correct_fuse_grid) and of
correct_batch's host assembly, written from behaviour: plain python / numpy.  Shared by tests/test_correct_grid_cpu.py and the GPU
tests of the grid."""
import numpy as np

from tests.correct_ref import fuse_ref


def mask_grid_ref(hyp, ntok, conf, frame, ths, mask_id, pad_id=0):
    """hyp [B,T], ntok [B], conf f32 [B,T], frame [B,T], ths [NT] -> (ys [NT,B,T], num_masked [NT,B], lm_rows, asr_rows): a token is
    masked where conf < th in f32, strictly; the lists run in (threshold, utterance, token) order"""
    hyp, conf, frame = np.asarray(hyp), np.asarray(conf, np.float32), np.asarray(frame)
    B, T = hyp.shape
    NT = len(ths)
    ys = np.full((NT, B, T), pad_id, np.int64)
    num = np.zeros((NT, B), np.int64)
    lm_rows, asr_rows = [], []
    for k, th in enumerate(np.asarray(ths, np.float32)):
        for b in range(B):
            for j in range(min(max(int(ntok[b]), 0), T)):
                if conf[b, j] < th:
                    ys[k, b, j] = mask_id
                    num[k, b] += 1
                    lm_rows.append((k * B + b) * T + j)
                    asr_rows.append(b * T + int(frame[b, j]))
                else:
                    ys[k, b, j] = hyp[b, j]
    return ys, num, np.asarray(lm_rows, np.int64), np.asarray(asr_rows, np.int64)


def fuse_grid_ref(asr, lm, ws, n_cols):
    """fuse_ref per weight -> (ids [NW,n], values [NW,n], margins [NW,n])"""
    out = [fuse_ref(asr, lm, float(w), n_cols) for w in ws]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def assemble_ref(hyp, positions, y_gen, pad_id=0):
    """hyp with y_gen at the masked positions, pad ids dropped (correct_batch's last step)"""
    cor = np.array(hyp, np.int64)
    cor[np.asarray(positions, np.int64)] = y_gen
    return [int(x) for x in cor if x != pad_id]
