"""Joint CTC / attention beam search with Transformer-LM shallow fusion on the GPU.

Behaviour follows TransformerDecoder.decode (asr/modeling/decoders/transformer.py:161-294)
including its quirks (see oracle/decoder.py:joint_beam_search): the LM term already sits inside
`scores_att` when the CTC re-scoring adds it again; finished hypotheses get
`score + len_weight * len(hyp incl. sos/eos)`; empty hypotheses are dropped; the search stops as
soon as `beam_width` results exist.

Device side per output step (all beams batched): decoder logits of the last position, LM
log-probabilities, log-softmax + fusion, top-k candidate selection, CTC prefix scores for every
(beam, candidate) with the scorer states kept on the device.  Host side: one small D2H per step
(candidate ids/scores), then the reference's own list bookkeeping (sort, prune, finish).

A stateful LM (the RNN LM, modeling/rnnlm.py) takes the host-bookkeeping path here (the batched device search steps it on the device
under decoder.joint_rnnlm_impl = "device"): every beam carries the slot of its LM state
(the LSTM run over hyp[:-1], as the reference's `lm_states`, decoders/transformer.py:190,223-253), an output step is ONE LM step
for all beams from the parents' slots into the other half of a double-buffered slot pool.
"""
import os

import numpy as np
import torch

from .. import ops
from ..engine import h2d_i32
from .functions import _engine_of
from .lm import require_next_token_lm

CTC_BEAM_WIDTH_RATIO = 1.5


def joint_beam_search(dec, eouts, elens, beam_width, len_weight=0, lm=None, lm_weight=0, decode_ctc_weight=0):
    require_next_token_lm(lm, lm_weight)
    eng = _engine_of(dec)
    assert eouts.shape[0] == 1, "beam search decodes one utterance at a time (decoders/transformer.py:181)"
    V, eos, blank = dec.vocab_size, dec.eos_id, dec.blank_id
    # the whole step on the device (K / V caches, device-side bookkeeping: one C-ABI call and one flag per step);
    # EMOASR_DEVICE_BEAM=0 keeps the host bookkeeping below (same results)
    if (os.environ.get("EMOASR_DEVICE_BEAM", "1") != "0" and os.environ.get("EMOASR_CPP_DECODE", "1") != "0"
            and beam_width <= 32 and min(V, int(beam_width * CTC_BEAM_WIDTH_RATIO)) <= 32
            and (lm is None or lm_weight <= 0 or hasattr(lm, "predict_device"))):
        from .beam_search_device import joint_beam_search_device
        return joint_beam_search_device(dec, eouts, elens, beam_width, len_weight, lm, lm_weight, decode_ctc_weight)
    dev = eouts.device
    T = eouts.shape[1]
    use_ctc = decode_ctc_weight > 0
    use_lm = lm is not None and lm_weight > 0
    lam, mu = float(decode_ctc_weight), float(lm_weight)
    with torch.no_grad():
        if use_ctc:
            ctc_logits = eng.head_logits(eouts, "decoder.ctc.output")
            x = ops.log_softmax(ctc_logits.view(T, V))
            init_state = ops.ctc_prefix_init(x, blank)
            cw = min(V, int(beam_width * CTC_BEAM_WIDTH_RATIO))
        # C++ step runtime (csrc/decode_rt.hip): one C-ABI call per network per output step, cross-attention
        # K / V of the memory projected once per utterance.  EMOASR_CPP_DECODE=0: per-kernel Python sequencing.
        rt = lmrt = None
        if os.environ.get("EMOASR_CPP_DECODE", "1") != "0":
            from ..decode_rt import DecoderStepRuntime, LMStepRuntime
            rt = getattr(eng, "_dec_rt", None)
            if rt is None:
                rt = eng._dec_rt = DecoderStepRuntime(eng)
            rt.begin(eouts, beam_width)
            if use_lm and hasattr(lm, "predict_device"):
                lmrt = getattr(lm, "_step_rt", None)
                if lmrt is None:
                    lmrt = lm._step_rt = LMStepRuntime(lm)
        side = None
        if lmrt is not None and os.environ.get("EMOASR_DECODE_STREAMS", "1") != "0":
            side = getattr(eng, "_lm_stream", None)
            if side is None:
                side = eng._lm_stream = torch.cuda.Stream(device=dev)
        beams = [dict(hyp=[eos], score=0.0, score_ctc=np.float32(0.0), parent=0, pcand=0, lm_slot=-1)]     # (-1: the zero state)
        stateful = use_lm and getattr(lm, "stateful", False)
        if stateful:
            pools = lm.new_pools(2 * beam_width, beam_width)

        def lm_rows(ys_in, i, nb):
            """f32 [nb, V]: the LM's next-token log-probabilities after every beam's hypothesis"""
            if not stateful:
                return lm.predict_device(ys_in, [i + 1] * nb)
            base = (i % 2) * beam_width     # this step's half of the pool; the beams' slots are in the other one
            ctl = h2d_i32([b["hyp"][-1] for b in beams] + [b["lm_slot"] for b in beams] + [base + m for m in range(nb)], dev)
            lm.step(pools, nb, ctl[:nb], ctl[nb:2 * nb], ctl[2 * nb:])
            return pools.logp[:nb]

        prev_states = None
        results = []
        for i in range(dec.max_decode_ylen):
            nb = len(beams)
            ys_in = torch.tensor([b["hyp"] for b in beams], dtype=torch.int64)
            if rt is not None:
                if lmrt is not None and side is not None:
                    # the LM and the decoder are independent chains of ~90 small kernels each: run the LM on a
                    # second stream so the two chains overlap (both are bound by the per-kernel dispatch floor)
                    main = torch.cuda.current_stream()
                    side.wait_stream(main)
                    with torch.cuda.stream(side), ops.stream_scope():
                        lm_lp = lmrt.step(ys_in)
                    with ops.stream_scope():
                        last = rt.step(ys_in)                                        # [nb, V]
                    main.wait_stream(side)
                    lm_lp.record_stream(main)
                else:
                    with ops.stream_scope():
                        last = rt.step(ys_in)
                        lm_lp = (lmrt.step(ys_in) if lmrt is not None else lm_rows(ys_in, i, nb)) if use_lm else None
            else:
                mem = eouts.expand(nb, T, eouts.shape[2]).contiguous()
                el = h2d_i32([T] * nb, dev)
                logits, _ = eng.dec_forward(mem, el, ys_in, [i] * nb, False, False)  # [nb, i+1, V]
                last = logits[:, i]
                lm_lp = lm_rows(ys_in, i, nb) if use_lm else None
            scores_pre = ops.log_softmax(last, add=lm_lp, mu=mu)  # = scores_att (+ lm: the in-place alias quirk)
            if use_ctc:
                vals, cands, lm_at = ops.topk(scores_pre, cw, aux=lm_lp)
                last_tok = h2d_i32([b["hyp"][-1] for b in beams], dev)
                out_len = h2d_i32([len(b["hyp"]) - 1 for b in beams], dev)
                parent = h2d_i32([b["parent"] for b in beams], dev)
                pcand = h2d_i32([b["pcand"] for b in beams], dev)
                log_psi, states = ops.ctc_prefix_score(x, cands, last_tok, out_len, blank, eos, prev_states, parent, pcand,
                                                       init_state)
                vals_h, cands_h, psi_h = vals.cpu().numpy(), cands.cpu().numpy(), log_psi.cpu().numpy()
                lm_h = lm_at.cpu().numpy() if use_lm else None
                prev_states = states
            else:
                vals, idx, _ = ops.topk(scores_pre, beam_width)
                vals_h, idx_h = vals.cpu().numpy(), idx.cpu().numpy()
            new_beams = []
            for m, beam in enumerate(beams):
                if use_ctc:
                    sc = np.float32(1 - lam) * vals_h[m] + np.float32(lam) * (psi_h[m] - beam["score_ctc"])
                    if use_lm:
                        sc = sc + np.float32(mu) * lm_h[m]
                    order = np.argsort(-sc, kind="stable")[:beam_width]
                    for j in order:
                        new_beams.append(dict(score=beam["score"] + float(sc[j]), hyp=beam["hyp"] + [int(cands_h[m, j])],
                                              score_ctc=psi_h[m, j], parent=m, pcand=int(j), lm_slot=(i % 2) * beam_width + m))
                else:
                    for j in range(beam_width):
                        new_beams.append(dict(score=beam["score"] + float(vals_h[m, j]), hyp=beam["hyp"] + [int(idx_h[m, j])],
                                              score_ctc=np.float32(0.0), parent=m, pcand=0, lm_slot=(i % 2) * beam_width + m))
            beams = sorted(new_beams, key=lambda b: b["score"], reverse=True)[:beam_width]
            alive = []
            for beam in beams:
                if beam["hyp"][-1] == eos:
                    hyp = [t for t in beam["hyp"] if t != eos]
                    if len(hyp) < 1:
                        continue
                    results.append(dict(hyp=hyp, score=beam["score"] + len_weight * len(beam["hyp"])))
                    if len(results) >= beam_width:
                        break
                else:
                    alive.append(beam)
            if len(results) >= beam_width or not alive:
                break
            beams = alive
    results = sorted(results, key=lambda r: r["score"], reverse=True)
    return [r["hyp"] for r in results], [r["score"] for r in results], None, None


def joint_beam_search_batch(dec, eouts, elens, beam_width, len_weight=0, lm=None, lm_weight=0, decode_ctc_weight=0):
    """the joint search for every utterance of a batch: eouts [B, Tmax, d], utterance b over its own elens[b] frames ->
    (hyps, scores, None, None), hyps[b] / scores[b] the lists joint_beam_search returns for eouts[b:b+1, :elens[b]].
    The batched device search (beam_search_device.joint_beam_search_device_batch: all searches in lockstep) takes it when it
    can; a stateful LM (the RNN LM) under dec.joint_rnnlm_impl = "host", beam_width or a candidate width above 32, and the switches
    that force the host bookkeeping fall back to one joint_beam_search per utterance.  joint_rnnlm_impl = "device" steps the RNN LM
    inside the batched device search and raises ValueError where that form cannot take the configuration."""
    require_next_token_lm(lm, lm_weight)
    lens = [int(n) for n in elens]
    if len(lens) != eouts.shape[0] or any(n < 1 for n in lens):
        raise ValueError(f"joint beam search: every utterance needs at least one encoder frame, got elens {lens}")
    from . import beam_search_device as bsd
    if bsd.batch_device_ok(dec, beam_width, lm, lm_weight, decode_ctc_weight):
        return bsd.joint_beam_search_device_batch(dec, eouts, lens, beam_width, len_weight, lm, lm_weight, decode_ctc_weight)
    hyps, scores = [], []
    for b, n in enumerate(lens):
        h, s, _, _ = joint_beam_search(dec, eouts[b:b + 1, :n], elens[b:b + 1], beam_width, len_weight, lm, lm_weight, decode_ctc_weight)
        hyps.append(h)
        scores.append(s)
    return hyps, scores, None, None
