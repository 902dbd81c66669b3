"""Restatements of the CTC error-correction step (emoasr_amd/correct.py, csrc/correct.hip), written from behaviour: plain python
over float64 arrays.  Shared by tests/test_correct_gpu.py and tests/test_p2w_cpu.py."""
import numpy as np


def collapse_runs(align, length, blank):
    """the tokens of a frame-level path: [(token id, [frames of its run])], a run = equal non-blank neighbours below `length`"""
    runs, prev = [], None
    for t in range(length):
        v = int(align[t])
        if v != blank:
            if v == prev:
                runs[-1][1].append(t)
            else:
                runs.append((v, [t]))
        prev = v
    return runs


def token_conf_ref(probs, align, length, blank):
    """probs [T, V] (softmax rows, float64) -> (ids, frames, confs, gaps): per token the first frame of its run where probs[t, id] is
    largest, that probability, and the relative distance to the run's second-best DISTINCT frame (inf for a one-frame run)"""
    ids, frames, confs, gaps = [], [], [], []
    for v, ts in collapse_runs(align, length, blank):
        p = np.asarray([probs[t, v] for t in ts], np.float64)
        k = int(np.argmax(p))     # the first maximum
        rest = np.delete(p, k)
        ids.append(v)
        frames.append(ts[k])
        confs.append(float(p[k]))
        gaps.append(float((p[k] - rest.max()) / p[k]) if len(rest) else float("inf"))
    return ids, frames, confs, gaps


def softmax64(z):
    z = np.asarray(z, np.float64)
    m = z.max(axis=-1, keepdims=True)
    e = np.exp(z - m)
    return e / e.sum(axis=-1, keepdims=True)


def fuse_ref(asr, lm, w, n_cols):
    """asr [n, V_asr], lm [n, V_lm] logits -> (ids, values, margins): first arg-max over v < n_cols of the mixed probabilities, the
    maximum, and its distance to the second-largest entry"""
    mix = (1.0 - w) * softmax64(asr)[:, :n_cols] + w * softmax64(lm)[:, :n_cols]
    ids = np.argmax(mix, axis=1)
    val = mix[np.arange(len(mix)), ids]
    if n_cols > 1:
        rest = mix.copy()
        rest[np.arange(len(mix)), ids] = -np.inf
        margin = val - rest.max(axis=1)
    else:
        margin = np.full(len(mix), np.inf)
    return ids, val, margin
