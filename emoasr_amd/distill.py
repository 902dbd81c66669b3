"""Soft labels for knowledge distillation from an LM teacher (asr/distill/make_label.py:30-210): the pickles
`{utt_id: [[(token, prob), ...], ...]}` that ASRDataset reads through params.kd_label_path.

    labels = make_bert_label("train_masked.tsv", bert_lm, save_path="train_bert_top8.pkl")     # columns utt_id, token_id, mask_pos
    labels = make_lm_label("train_spans.tsv", transformer_lm, save_path=...)                   # utt_id, token_id, start_pos, end_pos

BERT teacher: token_id already carries the mask token; one label per row, the teacher's distribution at mask_pos.  Transformer
teacher: one label per position of [start_pos, end_pos), the distribution after the tokens before it (row pos - 1); position 0 has
no left context and gets the hard label [(y[0], 1.0)].  With add_sos_eos the ids are wrapped in <eos> and the positions shift by
one -- unless the row is longer than max_seq_len - 2: then its first and last ids are REPLACED by <eos> and nothing shifts
("reduce context") -- and entries whose token is <eos> are dropped from the label without renormalising.  Several rows of one
utterance append to its list in file order.  A label is softmax(top-k logits / temp), k entries in descending order.

Device side, per batch of rows: ONE encoder forward (nothing stashed), the requested hidden rows gathered in chunks, transform +
vocabulary projection to f32 logits on those rows only, ops.topk (descending, ties to the lowest index), the soft-max over the k
survivors, and ONE device-to-host copy of the [M, k] ids and probabilities.  The offsets, the <eos> filter and the dict assembly
are host functions over those two arrays (plan_bert / plan_lm / assemble).
"""
import logging
import pickle

import numpy as np
import torch

from . import ops
from .datasets import _read_table
from .engine import h2d_i32

ROW_CHUNK = 4096     # gathered rows per transform + head call: [4096, V] f32 logits alive at a time


def _rows(rows):
    """a TSV path, a DataFrame or an iterable of dicts -> list of dicts"""
    if isinstance(rows, str):
        rows = _read_table(rows)
    if hasattr(rows, "to_dict") and hasattr(rows, "columns"):
        return rows.to_dict("records")
    return [dict(r) for r in rows]


def _ints(s):
    return [int(t) for t in s.split()] if isinstance(s, str) else [int(t) for t in s]


def _wrap(ids, add_sos_eos, eos_id, max_seq_len):
    """-> (ids of the teacher's input, shift of the row's positions)"""
    if not add_sos_eos:
        return ids, 0
    if len(ids) <= max_seq_len - 2:
        return [eos_id] + ids + [eos_id], 1
    return [eos_id] + ids[1:-1] + [eos_id], 0     # reduce context


def plan_bert(rows, add_sos_eos=False, eos_id=2, max_seq_len=256):
    """rows of (utt_id, token_id, mask_pos) -> (seqs, plan): the teacher's input sequences and, in output order, one request
    (utt_id, sequence index, position whose distribution is the label, None) per row"""
    seqs, plan = [], []
    for b, row in enumerate(rows):
        ids, shift = _wrap(_ints(row["token_id"]), add_sos_eos, eos_id, max_seq_len)
        assert len(ids) <= max_seq_len
        seqs.append(ids)
        plan.append((row["utt_id"], b, int(row["mask_pos"]) + shift, None))
    return seqs, plan


def plan_lm(rows, add_sos_eos=False, eos_id=2, max_seq_len=256):
    """rows of (utt_id, token_id, start_pos, end_pos) -> (seqs, plan): one request (utt_id, sequence index, pos - 1, None) per
    position pos of [start_pos, end_pos) (shifted as the ids are), or (utt_id, sequence index, None, y[0]) for pos == 0"""
    seqs, plan = [], []
    for b, row in enumerate(rows):
        ids, shift = _wrap(_ints(row["token_id"]), add_sos_eos, eos_id, max_seq_len)
        seqs.append(ids)
        for pos in range(int(row["start_pos"]) + shift, int(row["end_pos"]) + shift):
            if pos == 0:
                logging.warning(f"hard label is used: {ids[0]}")
                plan.append((row["utt_id"], b, None, ids[0]))
            else:
                plan.append((row["utt_id"], b, pos - 1, None))
    return seqs, plan


def assemble(labels, plan, ids, probs, add_sos_eos=False, eos_id=2):
    """append the plan's labels to the dict: ids / probs [M, k] hold the teacher's top-k of the plan's M soft requests, in plan order"""
    m = 0
    for utt_id, _, pos, hard in plan:
        if pos is None:
            pairs = [(int(hard), 1.0)]
        else:
            pairs = [(int(v), float(p)) for v, p in zip(ids[m], probs[m])]
            m += 1
        # NOTE: <eos> is not added to soft labels (and the rest is not renormalised)
        labels.setdefault(utt_id, []).append([(v, p) for v, p in pairs if not (add_sos_eos and v == eos_id)])
    assert m == len(ids), (m, len(ids))
    return labels


def teacher_topk(model, seqs, plan, topk, temp, want_logits=False):
    """one forward of the teacher over the padded sequences, the plan's soft requests only through transform + head
    -> (ids int64 [M, k], probs float32 [M, k]) on the host (+ the f32 logits [M, V] the top-k was taken of, for tests)"""
    if getattr(model, "lm_type", None) not in ("transformer", "bert"):
        raise NotImplementedError(f"emoasr_amd: soft labels from lm_type={getattr(model, 'lm_type', None)!r} are not provided")
    B, N = len(seqs), max(len(s) for s in seqs)
    ys = torch.zeros(B, N, dtype=torch.int64)
    for b, s in enumerate(seqs):
        ys[b, : len(s)] = torch.tensor(s)
    ys, yl = model._inputs(ys, [len(s) for s in seqs])
    flat = [b * N + pos for _, b, pos, _ in plan if pos is not None]
    for _, b, pos, _ in plan:
        assert pos is None or 0 <= pos < yl[b], f"position {pos} outside sequence {b} of length {yl[b]}"
    M, k = len(flat), int(topk)
    if M == 0:
        return np.zeros((0, k), np.int64), np.zeros((0, k), np.float32), *((np.zeros((0, 0), np.float32),) if want_logits else ())
    A = model._prepare()
    dev = A.flat.device
    kept = []
    with torch.no_grad(), ops.stream_scope(model._split()):
        x, _ = model._encode(h2d_i32(ys, dev), h2d_i32(yl, dev), B, N, 0.0, 0.0, False)
        sel = h2d_i32(flat, dev)
        W, bias = A.w(model._PRE + "embeddings.word_embeddings.weight"), A.p(model._CP + "bias")
        packed = torch.empty(M, 2 * k, device=dev, dtype=torch.int32)     # ids | probabilities (bit patterns): one copy back
        for m0 in range(0, M, ROW_CHUNK):
            t2, _ = model._transform(x.index_select(0, sel[m0:m0 + ROW_CHUNK]), False)
            logits = ops.gemm_nt(t2, W, bias=bias, out_f32=t2.dtype != torch.float32)
            vals, idx, _ = ops.topk(logits, k)
            probs = ops.log_softmax(ops.scale_dropout(vals, 1.0 / temp)).exp_()
            packed[m0:m0 + ROW_CHUNK, :k] = idx
            packed[m0:m0 + ROW_CHUNK, k:] = probs.view(torch.int32)
            if want_logits:
                kept.append(logits)
    host = packed.cpu()
    out = host[:, :k].to(torch.int64).numpy(), host[:, k:].contiguous().view(torch.float32).numpy()
    return out + (torch.cat(kept).cpu().numpy(),) if want_logits else out


def _make(planner, rows, model, save_path, topk, temp, add_sos_eos, eos_id, max_seq_len, batch_size):
    rows, labels = _rows(rows), {}
    for r0 in range(0, len(rows), batch_size):
        seqs, plan = planner(rows[r0:r0 + batch_size], add_sos_eos, eos_id, max_seq_len)
        ids, probs = teacher_topk(model, seqs, plan, topk, temp)
        assemble(labels, plan, ids, probs, add_sos_eos, eos_id)
    if save_path is not None:
        with open(save_path, "wb") as f:
            pickle.dump(labels, f)
        logging.info(f"pickle is saved to {save_path}")
    return labels


def make_bert_label(rows, model, save_path=None, topk=8, temp=3.0, add_sos_eos=False, eos_id=2, max_seq_len=256, batch_size=100):
    """make_label.py:126-210 -> {utt_id: [[(token, prob), ...], ...]} (pickled to save_path when one is given)"""
    return _make(plan_bert, rows, model, save_path, topk, temp, add_sos_eos, eos_id, max_seq_len, batch_size)


def make_lm_label(rows, model, save_path=None, topk=8, temp=3.0, add_sos_eos=False, eos_id=2, max_seq_len=256, batch_size=100):
    """make_label.py:30-123 -> {utt_id: [[(token, prob), ...], ...]} (pickled to save_path when one is given)"""
    return _make(plan_lm, rows, model, save_path, topk, temp, add_sos_eos, eos_id, max_seq_len, batch_size)
