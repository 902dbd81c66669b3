"""CTC error correction with a masked LM -- the protocol of asr/test_asr_correct.py:39-232 on the HIP path.

    frame, conf, ntok = token_confidences(logits, best, elens, blank_id)
    utt_id, hyp, hyp_cor, reftext, num_masked, num_tokens = correct_step(model, lm, data, blank_id, mask_id, mask_th, lm_weight,
                                                                         device, vocab_size)
    rows = test(model, lm, dataloader, vocab, vocab_size, device, blank_id, mask_id, mask_th, lm_weight)
    cells = correct_batch(model, lm, data, blank_id, mask_id, mask_ths, lm_weights, device, vocab_size)     # any batch size, a grid

The recogniser's greedy path is collapsed into tokens; a token's confidence is the largest soft-max probability of its id over the
frames of its run (ops.ctc_token_conf, csrc/correct.hip).  Tokens below `mask_th` become `mask_id`; the LM -- an LM with
lm_type "bert", or a P2W "pbert" given the phone hypothesis -- reads the masked hypothesis, and at the masked positions the new token
is argmax_v (1 - w) p_asr[v] + w p_lm[v] over v < vocab_size (ops.correct_fuse), p_asr the recogniser's soft-max at the token's most
confident frame.  "pctc" is the cascade: the phone hypothesis goes through P2W.decode.

One encoder pass per utterance feeds the word and the phone head.  No soft-max row is formed outside the kernels; the host sees the
greedy ids, confidences and counts (one copy: the LM modules take their input ids from the host) and the fused ids (one copy).

correct_batch is the same protocol for a padded batch and a grid of (mask_th, lm_weight) cells: the masked inputs of every threshold
are built on the device (ops.correct_mask_grid), the LM reads them there (LM.logits_at / P2W.logits_at: the vocabulary product on
the masked rows alone), and one ops.correct_fuse_grid launch fuses all weights (at most 16 per launch; ops chunks above that).
"""
import logging

import numpy as np
import torch

from . import ops
from .decode import ints2str
from .modeling.functions import _elens_dev


def token_confidences(logits, aligns_or_best, elens, blank_id):
    """logits [B,T,V] (device); aligns_or_best: the greedy frame ids as an int tensor [B,T] or as the per-utterance lists that
    decode() returns; elens [B] -> (frame int32 [B,T], conf f32 [B,T], ntok int32 [B]) on the device (ops.ctc_token_conf)"""
    B, T, V = logits.shape
    dev = logits.device
    if torch.is_tensor(aligns_or_best):
        best = aligns_or_best.to(device=dev, dtype=torch.int32).contiguous()
    else:
        host = torch.full((B, T), int(blank_id), dtype=torch.int32)
        for b, a in enumerate(aligns_or_best):
            host[b, :len(a)] = torch.as_tensor(a, dtype=torch.int32)
        best = host.to(dev)
    el = torch.as_tensor(elens).to(device=dev, dtype=torch.int32)
    if not logits.is_contiguous() and not (logits.stride(2) == 1 and logits.stride(0) == T * logits.stride(1)):
        logits = logits.contiguous()
    lse = ops.row_lse(logits.reshape(B * T, V) if logits.is_contiguous() else logits.view(B * T, V))
    return ops.ctc_token_conf(logits, lse, best, el, blank_id)


def _is_p2w(lm):
    return getattr(lm, "lm_type", None) in ("pbert", "pctc")


def correct_step(model, lm, data, blank_id, mask_id, mask_th, lm_weight, device, vocab_size, pad_id=0, cascade_ctc=False,
                 details=None):
    """test_step of asr/test_asr_correct.py:75-172 for the (single-utterance) batch `data`
    -> (utt_id, hyp, hyp_cor, reftext, num_masked, num_tokens).  details: a dict that receives hyp_phone, token_probs_v,
    hyp_masked, mask_indices, mix_values (the fused maxima) and y_gen of the step, and the device tensors the kernels read
    (asr_logits [T', V], best [T'], lse [T'], frames [n], lm_logits [n, V_lm])."""
    utt_id = data["utt_ids"][0]
    reftext = data["texts"][0]
    xs = data["xs"].to(device)
    xlens = data["xlens"]
    use_phone = _is_p2w(lm)
    dec = model.decoder
    with torch.no_grad():
        eouts, elens, eouts_inter = model.encoder(xs, xlens)      # ONE encoder pass for both heads
        assert eouts.shape[0] == 1, "correction decodes one utterance at a time (test_asr_correct.py:91)"
        eng = model.engine()
        el = _elens_dev(eouts, elens)
        T = eouts.shape[1]
        logits = eng.head_logits(eouts, dec._prefix + ".output", out_f32=eng.f32_head)
        best, hyp_d, hyplen = eng.greedy(logits, el, blank_id)
        parts = [hyplen.view(-1)[:1], hyp_d.view(-1)[:T]]
        if use_phone:
            src = eouts_inter if dec.hie_mtl_phone else eouts
            plogits = eng.head_logits(src, dec._prefix + ".phone_output", out_f32=eng.f32_head)
            _, phyp_d, phyplen = eng.greedy(plogits, el, blank_id)
            parts += [phyplen.view(-1)[:1], phyp_d.view(-1)[:T]]
        if not cascade_ctc:
            V = logits.shape[-1]
            lse = ops.row_lse(logits.view(T, V))
            frame, conf, _ = ops.ctc_token_conf(logits, lse, best.contiguous(), el, blank_id)
            parts += [conf.view(-1).view(torch.int32)]
        host = torch.cat(parts).cpu().numpy()                     # the step's one copy of ids, counts and confidences
    n = int(host[0])
    hyp = host[1:1 + n].astype(np.int64)
    off = 1 + T
    hyp_phone = None
    if use_phone:
        n_p = int(host[off])
        hyp_phone = host[off + 1:off + 1 + n_p].astype(np.int64)
        off += 1 + T
    if details is not None:
        details.update(hyp_phone=hyp_phone)
    if n < 1 or (use_phone and len(hyp_phone) < 1):
        return utt_id, [], [], reftext, 0, 0
    if cascade_ctc:
        hyp_cor = lm.decode(ps=torch.as_tensor(hyp_phone).unsqueeze(0))[0]
        return utt_id, hyp, hyp_cor, reftext, 0, 0
    token_probs_v = host[off:off + n].view(np.float32)
    mask_indices = token_probs_v < mask_th
    hyp_masked = hyp.copy()
    hyp_masked[mask_indices] = mask_id
    num_masked, num_tokens = int(mask_indices.sum()), int(len(mask_indices))
    with torch.no_grad():
        y = torch.as_tensor(hyp_masked).unsqueeze(0)
        lm_logits = lm(y, ps=torch.as_tensor(hyp_phone).unsqueeze(0)) if use_phone else lm(y)
        ids, val = ops.correct_fuse(logits.view(T, -1), lse, lm_logits[0], lm_weight, vocab_size,
                                    asr_rows=frame.view(-1)[:n].contiguous())
        fused = torch.cat([ids, val.view(torch.int32)]).cpu().numpy()     # the fused ids (and their values)
    y_gen = fused[:n].astype(np.int64)
    hyp_cor = hyp.copy()
    hyp_cor[mask_indices] = y_gen[mask_indices]
    hyp_cor = [int(x) for x in hyp_cor if x != pad_id]
    if details is not None:
        details.update(token_probs_v=token_probs_v, hyp_masked=hyp_masked, mask_indices=mask_indices,
                       mix_values=fused[n:].view(np.float32), y_gen=y_gen, asr_logits=logits[0], best=best[0], lse=lse,
                       frames=frame.view(-1)[:n], lm_logits=lm_logits[0])
    return utt_id, hyp, hyp_cor, reftext, num_masked, num_tokens


def _grid_axis(v):
    return [float(x) for x in (v if isinstance(v, (list, tuple, np.ndarray)) else [v])]


def correct_batch(model, lm, data, blank_id, mask_id, mask_ths, lm_weights, device, vocab_size, pad_id=0, cascade_ctc=False,
                  details=None):
    """correct_step for a collated batch of any size and a grid of cells (mask_th, lm_weight); scalars are one-entry axes
    -> cells[k][m] = the list of correct_step's tuples, one per utterance, for mask_ths[k] and lm_weights[m].

    ONE recogniser pass (with engine.mask_padding: every utterance of the padded batch gets the encoder output, hence the tuples,
    it gets alone) and one pass of the greedy / confidence kernels for the whole grid; ops.correct_mask_grid builds the masked
    inputs and the row lists of every threshold; ONE LM pass per masked input, i.e. per threshold that masks something
    (lm.logits_at over the stacked inputs: the vocabulary product runs on the masked rows alone, a P2W's phone encoder once per
    utterance); ONE ops.correct_fuse_grid over all weights.  Two device-to-host copies per batch: the counts (to size the LM call),
    then the ids.  An utterance whose word hypothesis (or phone hypothesis, for a P2W) is empty yields (utt_id, [], [], reftext, 0, 0)
    in every cell.  cascade_ctc ("pctc"): one batched P2W.decode over the padded phone hypotheses, no grid: one cell.

    details: a dict that receives the device tensors the kernels read (asr_logits [B,T',V], lse, best, hyp, ntok, conf, frames, ths,
    ys, num_masked, lm_rows, asr_rows, lm_logits), the host lists hyp_phone[b], hyp_masked[k][b], mask_positions[k][b], y_gen[k][m][b]
    and mix_values[k][m][b] (the fused ids and maxima at the masked positions), valid[b], and lm_calls (masked inputs passed
    through the LM)."""
    ths, ws = _grid_axis(mask_ths), _grid_axis(lm_weights)
    NT, NW = len(ths), len(ws)
    utt_ids, reftexts = list(data["utt_ids"]), list(data["texts"])
    xs = data["xs"].to(device)
    B = xs.shape[0]
    use_phone = _is_p2w(lm)
    dec = model.decoder
    empty = lambda b: (utt_ids[b], [], [], reftexts[b], 0, 0)
    with torch.no_grad():
        # ONE encoder pass for both heads and every cell.  The convolution module masks the padded frames for this pass, so a padded
        # utterance gets the hypothesis it gets alone, i.e. correct_step's (engine.mask_padding; off everywhere else, as the reference)
        eng = model.engine()
        keep = getattr(eng, "mask_padding", False)
        eng.mask_padding = B > 1
        try:
            eouts, elens, eouts_inter = model.encoder(xs, data["xlens"])
        finally:
            eng.mask_padding = keep
        el = _elens_dev(eouts, elens)
        T = eouts.shape[1]
        logits = eng.head_logits(eouts, dec._prefix + ".output", out_f32=eng.f32_head)
        best, hyp_d, hyplen = eng.greedy(logits, el, blank_id)
        phyp_d = phyplen = None
        if use_phone:
            src = eouts_inter if dec.hie_mtl_phone else eouts
            plogits = eng.head_logits(src, dec._prefix + ".phone_output", out_f32=eng.f32_head)
            _, phyp_d, phyplen = eng.greedy(plogits, el, blank_id)
        if cascade_ctc:
            host = torch.cat([hyplen, phyplen, hyp_d.reshape(-1), phyp_d.reshape(-1)]).cpu().numpy()     # the batch's one copy
            n_w, n_p = host[:B], host[B:2 * B]
            hyps = host[2 * B:2 * B + B * T].reshape(B, T).astype(np.int64)
            phyps = host[2 * B + B * T:].reshape(B, T).astype(np.int64)
            valid = [b for b in range(B) if n_w[b] >= 1 and n_p[b] >= 1]
            out = [empty(b) for b in range(B)]
            if valid:
                ps = torch.zeros(len(valid), int(max(n_p[b] for b in valid)), dtype=torch.int64)
                for i, b in enumerate(valid):
                    ps[i, :n_p[b]] = torch.from_numpy(phyps[b, :n_p[b]])
                cor = lm.decode(ps=ps, plens=[int(n_p[b]) for b in valid])
                for i, b in enumerate(valid):
                    out[b] = (utt_ids[b], hyps[b, :n_w[b]], cor[i], reftexts[b], 0, 0)
            if details is not None:
                details.update(hyp_phone=[phyps[b, :n_p[b]] for b in range(B)], lm_calls=0)
            return [[out]]
        V = logits.shape[-1]
        lse = ops.row_lse(logits.view(B * T, V))
        frame, conf, ntok = ops.ctc_token_conf(logits, lse, best.contiguous(), el, blank_id)
        ths_dev = torch.tensor(ths, dtype=torch.float32).pin_memory().to(logits.device, non_blocking=True)
        ys, num_masked, lm_rows, asr_rows = ops.correct_mask_grid(hyp_d.contiguous(), ntok, conf, frame, ths_dev, mask_id, pad_id)
        counts = torch.cat([ntok] + ([phyplen] if use_phone else []) + [num_masked.view(-1)]).cpu().numpy()     # copy 1: the counts
        n_w = counts[:B]
        n_p = counts[B:2 * B] if use_phone else None
        nm = counts[-NT * B:].reshape(NT, B)
        valid = [bool(n_w[b] >= 1 and (not use_phone or n_p[b] >= 1)) for b in range(B)]
        total = int(nm.sum())
        active = [k for k in range(NT) if nm[k].sum() > 0]
        lm_logits = ids = vals = None
        rows, arows = lm_rows[:total], asr_rows[:total]
        if total:
            # the LM reads the inputs of the thresholds that mask something, stacked [len(active) * B, T]; lengths of 0 go in as 1
            # (a pad token nobody reads: such an utterance has no masked row, or is dropped below)
            ys_in, rows_in = ys.view(NT * B, T), rows
            if len(active) < NT:
                sel = torch.tensor(active, dtype=torch.int64).pin_memory().to(ys.device, non_blocking=True)
                shift = torch.zeros(NT, dtype=torch.int32)
                for i, k in enumerate(active):
                    shift[k] = (k - i) * B * T
                ys_in = ys.index_select(0, sel).view(len(active) * B, T)
                rows_in = rows - shift.pin_memory().to(ys.device, non_blocking=True)[(rows // (B * T)).long()]
            ylens = [max(int(v), 1) for v in n_w] * len(active)
            if use_phone:
                keep = torch.arange(T, device=phyp_d.device).unsqueeze(0) < phyplen.unsqueeze(1)
                ps = torch.where(keep, phyp_d, torch.zeros_like(phyp_d))      # (ids past a hypothesis' end are unset)
                lm_logits = lm.logits_at(ys_in, ylens, rows_in, ps, [max(int(v), 1) for v in n_p])
            else:
                lm_logits = lm.logits_at(ys_in, ylens, rows_in)
            ids, vals = ops.correct_fuse_grid(logits.view(B * T, V), lse, lm_logits, ws, vocab_size, asr_rows=arows.contiguous())
        parts = [hyp_d.reshape(-1)] + ([phyp_d.reshape(-1)] if use_phone else [])
        if total:
            parts += [rows, ids.view(-1), vals.view(-1).view(torch.int32)]
        host = torch.cat(parts).cpu().numpy()                             # copy 2: hypotheses, masked positions, fused ids
    hyps = host[:B * T].reshape(B, T).astype(np.int64)
    off = B * T
    phyps = None
    if use_phone:
        phyps = host[off:off + B * T].reshape(B, T).astype(np.int64)
        off += B * T
    pos = host[off:off + total] % T
    y_gen = host[off + total:off + total + NW * total].reshape(NW, total).astype(np.int64)
    mix = host[off + total + NW * total:].view(np.float32).reshape(NW, total)
    first = np.concatenate([[0], np.cumsum(nm.reshape(-1))])              # the lists' order: (threshold, utterance, token)
    cells = [[[] for _ in ws] for _ in ths]
    det = dict(hyp_masked=[], mask_positions=[], y_gen=[[[] for _ in ws] for _ in ths], mix_values=[[[] for _ in ws] for _ in ths])
    for k in range(NT):
        det["hyp_masked"].append([])
        det["mask_positions"].append([])
        for b in range(B):
            lo, hi = int(first[k * B + b]), int(first[k * B + b + 1])
            hyp = hyps[b, :n_w[b]]
            masked = hyp.copy()
            masked[pos[lo:hi]] = mask_id
            det["hyp_masked"][k].append(masked)
            det["mask_positions"][k].append(pos[lo:hi])
            for m in range(NW):
                det["y_gen"][k][m].append(y_gen[m, lo:hi])
                det["mix_values"][k][m].append(mix[m, lo:hi])
                if not valid[b]:
                    cells[k][m].append(empty(b))
                    continue
                cor = hyp.copy()
                cor[pos[lo:hi]] = y_gen[m, lo:hi]
                cells[k][m].append((utt_ids[b], hyp, [int(x) for x in cor if x != pad_id], reftexts[b], hi - lo, int(n_w[b])))
    if details is not None:
        details.update(det, asr_logits=logits, lse=lse, best=best, hyp=hyp_d, ntok=ntok, conf=conf, frames=frame, ths=ths_dev, ys=ys,
                       num_masked=num_masked, lm_rows=rows, asr_rows=arows, lm_logits=lm_logits, valid=valid,
                       lm_calls=len(active) if total else 0,
                       hyp_phone=[phyps[b, :n_p[b]] for b in range(B)] if use_phone else None)
    return cells


def test(model, lm, dataloader, vocab, vocab_size, device, blank_id, mask_id, mask_th, lm_weight, pad_id=0, num_samples=-1,
         cascade_ctc=False, impl=None):
    """test of asr/test_asr_correct.py:175-232 -> result rows [utt_id, token_id, text, reftext] (the shape decode.test writes).  A
    batch of several utterances goes through correct_batch; a batch of one through correct_step unless impl="batch"."""
    if impl not in (None, "step", "batch"):
        raise ValueError(f"impl {impl!r}: None, 'step' or 'batch'")
    rows = []
    num_masked_all = num_tokens_all = 0
    for i, data in enumerate(dataloader):
        if num_samples > 0 and (i + 1) > num_samples:
            return rows
        if len(data["utt_ids"]) > 1 or impl == "batch":
            steps = correct_batch(model, lm, data, blank_id, mask_id, mask_th, lm_weight, device, vocab_size, pad_id=pad_id,
                                  cascade_ctc=cascade_ctc)[0][0]
        else:
            steps = [correct_step(model, lm, data, blank_id, mask_id, mask_th, lm_weight, device, vocab_size, pad_id=pad_id,
                                  cascade_ctc=cascade_ctc)]
        for utt_id, hyp, hyp_cor, reftext, num_masked, num_tokens in steps:
            num_masked_all += num_masked
            num_tokens_all += num_tokens
            if len(hyp) < 1:
                token_id, text = None, ""
                logging.warning(f"cannot decode {utt_id}")
            else:
                token_id, text = ints2str(hyp_cor), vocab.ids2text(hyp_cor)
            rows.append([utt_id, token_id, text, reftext])
    logging.info(f"masked: {num_masked_all:d} / {num_tokens_all:d}")
    return rows
