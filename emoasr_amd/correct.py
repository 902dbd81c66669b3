"""CTC error correction with a masked LM -- the protocol of asr/test_asr_correct.py:39-232 on the HIP path.

    frame, conf, ntok = token_confidences(logits, best, elens, blank_id)
    utt_id, hyp, hyp_cor, reftext, num_masked, num_tokens = correct_step(model, lm, data, blank_id, mask_id, mask_th, lm_weight,
                                                                         device, vocab_size)
    rows = test(model, lm, dataloader, vocab, vocab_size, device, blank_id, mask_id, mask_th, lm_weight)

The recogniser's greedy path is collapsed into tokens; a token's confidence is the largest soft-max probability of its id over the
frames of its run (ops.ctc_token_conf, csrc/correct.hip).  Tokens below `mask_th` become `mask_id`; the LM -- an LM with
lm_type "bert", or a P2W "pbert" given the phone hypothesis -- reads the masked hypothesis, and at the masked positions the new token
is argmax_v (1 - w) p_asr[v] + w p_lm[v] over v < vocab_size (ops.correct_fuse), p_asr the recogniser's soft-max at the token's most
confident frame.  "pctc" is the cascade: the phone hypothesis goes through P2W.decode.

One encoder pass per utterance feeds the word and the phone head.  No soft-max row is formed outside the kernels; the host sees the
greedy ids, confidences and counts (one copy: the LM modules take their input ids from the host) and the fused ids (one copy).
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


def test(model, lm, dataloader, vocab, vocab_size, device, blank_id, mask_id, mask_th, lm_weight, pad_id=0, num_samples=-1,
         cascade_ctc=False):
    """test of asr/test_asr_correct.py:175-232 -> result rows [utt_id, token_id, text, reftext] (the shape decode.test writes)"""
    rows = []
    num_masked_all = num_tokens_all = 0
    for i, data in enumerate(dataloader):
        if num_samples > 0 and (i + 1) > num_samples:
            return rows
        utt_id, hyp, hyp_cor, reftext, num_masked, num_tokens = correct_step(
            model, lm, data, blank_id, mask_id, mask_th, lm_weight, device, vocab_size, pad_id=pad_id, cascade_ctc=cascade_ctc)
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
