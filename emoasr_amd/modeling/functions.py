"""autograd glue: two Functions connect the engine's explicit forward/backward to
`loss.backward()`, one for the encoder stack and one for the CTC head, so the
encoder/decoder module boundary of the reference survives.

Parameter gradients are accumulated by the engine directly into the flat gradient arena
(the parameters' .grad tensors are views of it); the Functions therefore return None for
the parameter inputs.
"""
import logging

import torch

from .. import lockstep
from ..engine import h2d_i32


def _engine_of(mod):
    if mod._owner is None:
        raise RuntimeError("emoasr_amd: encoder/decoder modules run through their owning ASR model")
    return mod._owner[0].engine()


def _host_list(lens):
    if torch.is_tensor(lens):
        return lens.tolist()  # device tensors sync here, like max(xlens) in asr.py:57
    return [int(v) for v in lens]


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, training, xs, xlens_host, *params):
        eouts, elens_host, elens_dev, st = eng.forward(xs, xlens_host, training, stash=True)
        ctx.eng, ctx.st = eng, st
        ctx.mark_non_differentiable(elens_dev)
        inter = eng.eouts_inter
        ctx.has_inter = inter is not None
        if inter is None:
            inter = eouts.new_empty(0)
            ctx.mark_non_differentiable(inter)
        return eouts, elens_dev, inter

    @staticmethod
    def backward(ctx, deouts, _, dinter):
        ctx.eng.backward(ctx.st, deouts.contiguous(), dinter.contiguous() if ctx.has_inter else None)
        ctx.st = None
        return (None,) * (4 + len(ctx.eng.arena.params))


def encoder_apply(enc, xs, xlens):
    eng = _engine_of(enc)
    host = _host_list(xlens)
    embed = getattr(enc, "input_layer", "conv2d") == "embed"
    if embed:      # token ids [B, P]: they go up as int32 from pinned memory
        ids = (xs.cpu() if torch.is_tensor(xs) else torch.as_tensor(xs)).to(torch.int64)
        assert ids.dim() == 2 and 0 <= int(ids.min()) and int(ids.max()) < enc.embed.num_embeddings, "phone id outside the vocabulary"
        assert len(host) == ids.shape[0] and 1 <= min(host) and max(host) <= ids.shape[1], "plens: one length in [1, P] per row"
        xs = h2d_i32(ids.contiguous(), enc.embed.weight.device)
    else:
        xs = xs.to(torch.float32).contiguous()
    if torch.is_grad_enabled():
        eng.step_count += 1
        eouts, elens_dev, inter = _EncoderFn.apply(eng, enc.training, xs, host, *eng.arena.params)
        inter = inter if eng.eouts_inter is not None else None
    else:
        eouts, _, elens_dev, _ = eng.forward(xs, host, enc.training, stash=False)
        inter = eng.eouts_inter
    elens = torch.tensor(host if embed else [((v - 1) // 2 - 1) // 2 for v in host], dtype=torch.int64)
    if torch.is_tensor(xlens):
        elens = elens.to(xlens.device)
    eouts._emo_elens_dev = elens_dev
    if inter is not None:
        inter._emo_elens_dev = elens_dev
    return eouts, elens, inter


def rnn_encoder_apply(enc, xs, xlens):
    """RNNEncoder.forward on the engine (engine/rnn_encoder.py) -> (eouts [B, max elens, H], elens, None); the output length and the
    lengths are pad_packed_sequence's (input_layer "none": elens = xlens)"""
    eng = _engine_of(enc)
    xs = xs.to(torch.float32).contiguous()
    host = _host_list(xlens)
    if torch.is_grad_enabled():
        eng.step_count += 1
        eouts, elens_dev, _ = _EncoderFn.apply(eng, enc.training, xs, host, *eng.arena.params)
    else:
        eouts, _, elens_dev, _ = eng.forward(xs, host, enc.training, stash=False)
    elens = torch.tensor(eng._rnn_elens(host), dtype=torch.int64)
    if torch.is_tensor(xlens):
        elens = elens.to(xlens.device)
    eouts._emo_elens_dev = elens_dev
    return eouts, elens, None


class _EncoderStackedFn(torch.autograd.Function):
    """the encoder over several micro-batches in ONE stacked pass (engine.encoder_forward_stacked): outputs one eouts tensor per
    micro-batch (views of the stacked rows); the backward waits for all of their gradients and runs one stacked sweep"""

    @staticmethod
    def forward(ctx, eng, n, *args):
        xs_list, xlens_list = list(args[:n]), list(args[n:2 * n])
        eouts, st = eng.encoder_forward_stacked(xs_list, xlens_list)
        ctx.eng, ctx.st = eng, st
        outs = tuple(eouts[st.rows[k]:st.rows[k + 1]].view(st.segs[k][0], st.segs[k][1], eouts.shape[1]) for k in range(n))
        return outs

    @staticmethod
    def backward(ctx, *grads):
        st = ctx.st
        eng = ctx.eng
        d = grads[0].shape[-1] if grads[0] is not None else eng.d
        deouts = torch.empty(st.M, d, device=st.y2.device, dtype=eng.dtype)
        for k, gk in enumerate(grads):
            dst = deouts[st.rows[k]:st.rows[k + 1]]
            if gk is None:
                dst.zero_()
            else:
                dst.copy_(gk.reshape(-1, d))
        eng.encoder_backward_stacked(st, deouts)
        ctx.st = None
        return (None, None) + (None,) * (len(grads) * 2 + len(eng.arena.params))


def encoder_apply_stacked(enc, xs_list, xlens_list):
    """TransformerEncoder.forward for several micro-batches at once (training, autograd on): -> [(eouts, elens, None), ...].
    Each micro-batch keeps its own padding, BatchNorm batch statistics and relative-position table (include/emoasr_hip.h:
    emoasr_segments_t); only the row-wise kernels see them together."""
    eng = _engine_of(enc)
    xs_list = [x.to(torch.float32).contiguous() for x in xs_list]
    hosts = [_host_list(v) for v in xlens_list]
    n = len(xs_list)
    outs = _EncoderStackedFn.apply(eng, n, *xs_list, *hosts, *eng.arena.params)
    res = []
    for k in range(n):
        elens = torch.tensor([((v - 1) // 2 - 1) // 2 for v in hosts[k]], dtype=torch.int64)
        eo = outs[k]
        # the decoders' device copy of the lengths, uploaded from pinned memory without waiting for the stream (a pageable
        # `.to(device)` here blocked the host behind the whole stacked encoder pass, once per micro-batch: the launch queue ran
        # dry five times per optimizer step)
        eo._emo_elens_dev = h2d_i32(elens.to(torch.int32), eo.device)
        res.append((eo, elens, None))
    return res


class _CTCLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, eouts, elens_dev, ys_host, ylens_host, blank, head, *params):
        logits = eng.head_logits(eouts, head)
        need = eouts.requires_grad or any(p.requires_grad for p in params)
        loss, cctx = eng.ctc_loss(logits, elens_dev, ys_host, ylens_host, blank, need)
        ctx.eng, ctx.cctx, ctx.eouts, ctx.head = eng, cctx, eouts, head
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, gloss, _):
        eng = ctx.eng
        gdev = gloss.to(torch.float32).reshape(1) if gloss.is_cuda else None  # no host sync
        dlogits = eng.ctc_grad(ctx.cctx, 1.0 if gdev is not None else float(gloss), gdev)
        deouts = eng.head_backward(ctx.eouts, dlogits, ctx.head)
        ctx.cctx = None
        return (None, deouts, None, None, None, None, None) + (None,) * len(eng.arena.params)


class _HeadFn(torch.autograd.Function):
    """a vocabulary head on its own (logits = eouts W^T + b), for losses that are separate autograd nodes"""

    @staticmethod
    def forward(ctx, eng, eouts, head, *params):
        ctx.eng, ctx.eouts, ctx.head = eng, eouts, head
        return eng.head_logits(eouts, head)

    @staticmethod
    def backward(ctx, dlogits):
        deouts = ctx.eng.head_backward(ctx.eouts, dlogits, ctx.head)
        return (None, deouts, None) + (None,) * len(ctx.eng.arena.params)


class _CTCLogitsFn(torch.autograd.Function):
    """CTC loss of given logits (+ optionally the forced alignment read off the same lattices)"""

    @staticmethod
    def forward(ctx, eng, logits, elens_dev, ys_host, ylens_host, blank, want_aligns):
        from .. import ops
        loss, cctx = eng.ctc_loss(logits, elens_dev, ys_host, ylens_host, blank, True)
        ctx.eng, ctx.cctx = eng, cctx
        if want_aligns:
            _, _, labels, elens, ylens, _, lp, alpha, beta, _ = cctx
            aligns = ops.ctc_best_path(lp, alpha, beta, labels, elens, ylens, blank)
        else:
            aligns = torch.empty(0, dtype=torch.int32, device=logits.device)
        ctx.mark_non_differentiable(aligns)
        return loss, aligns

    @staticmethod
    def backward(ctx, gloss, _):
        dlogits = ctx.eng.ctc_grad(ctx.cctx, 1.0, gloss.to(torch.float32).reshape(1))
        ctx.cctx = None
        return None, dlogits, None, None, None, None, None


def head_apply(dec, eouts, head):
    eng = _engine_of(dec)
    return _HeadFn.apply(eng, eouts, head, *eng.arena.params)


def ctc_from_logits_apply(dec, logits, eouts, elens, ys, ylens, want_aligns=False):
    """-> (loss_ctc = sum_b nll_b / B, aligns int32 [B,T] | None)"""
    eng = _engine_of(dec)
    ys_host = ys.cpu() if torch.is_tensor(ys) else torch.as_tensor(ys)
    loss, aligns = _CTCLogitsFn.apply(eng, logits, _elens_dev(eouts, elens), ys_host, _host_list(ylens), dec.blank_id,
                                      want_aligns)
    return loss, (aligns if want_aligns else None)


def ctc_forced_align_apply(log_probs, elens, ys, ylens, blank):
    """CTCForcedAligner.__call__ (ctc_aligner.py:139-221) on the CTC lattice kernels -> int64 [B,T] (device)"""
    from .. import ops
    dev = log_probs.device
    lp_in = log_probs.contiguous()
    B, T, V = lp_in.shape
    ylens_host = _host_list(ylens)
    Lmax = max(max(ylens_host), 1)
    labels = torch.as_tensor(ys)[:, :Lmax].to(torch.int32)
    if labels.shape[1] < Lmax:
        labels = torch.nn.functional.pad(labels, (0, Lmax - labels.shape[1]))
    labels = labels.contiguous().to(dev)
    el = torch.as_tensor(elens).to(torch.int32).to(dev)
    yl = torch.tensor(ylens_host, dtype=torch.int32).to(dev)
    with ops.stream_scope():
        lse = ops.row_lse(lp_in.view(B * T, V))
        lp, alpha, beta, _ = ops.ctc_forward(lp_in, lse, labels, el, yl, blank)
        return ops.ctc_best_path(lp, alpha, beta, labels, el, yl, blank).long()


def _elens_dev(eouts, elens):
    dev = getattr(eouts, "_emo_elens_dev", None)
    if dev is None:
        t = torch.as_tensor(elens)
        # (a host tensor goes up from pinned memory, asynchronously; a device tensor is converted in place on the stream)
        dev = t.to(torch.int32) if t.is_cuda else h2d_i32(t.to(torch.int32), eouts.device)
    return dev


def ctc_head_apply(dec, eouts, head="decoder.output"):
    return _engine_of(dec).head_logits(eouts, head)


def ctc_loss_apply(dec, eouts, elens, ys, ylens, head="decoder.output"):
    eng = _engine_of(dec)
    ys_host = ys.cpu() if torch.is_tensor(ys) else torch.as_tensor(ys)
    return _CTCLossFn.apply(eng, eouts, _elens_dev(eouts, elens), ys_host, _host_list(ylens), dec.blank_id, head,
                            *eng.arena.params)


def ctc_greedy_apply(dec, eouts, elens, head="output"):
    """greedy CTC decoding through the head `head` of the decoder ("output": words, "phone_output": phones)"""
    eng = _engine_of(dec)
    logits = eng.head_logits(eouts, getattr(dec, "_prefix", "decoder") + "." + head, out_f32=eng.f32_head)
    best, hyp, hyplen = eng.greedy(logits, _elens_dev(eouts, elens), dec.blank_id)
    B, T = best.shape
    packed = best._base.cpu() if best._base is not None and best._base.numel() == 2 * B * T + B else None   # one D2H per batch
    if packed is not None:
        best_h, hyp_h, n_h = packed[:B * T].view(B, T), packed[B * T:2 * B * T].view(B, T), packed[2 * B * T:].tolist()
    else:
        best_h, hyp_h, n_h = best.cpu(), hyp.cpu(), hyplen.cpu().tolist()
    el = _host_list(elens)
    hyps = [hyp_h[b, : n_h[b]].tolist() for b in range(len(n_h))]
    aligns = [best_h[b, : el[b]].tolist() for b in range(len(n_h))]
    return hyps, [None] * len(hyps), logits, aligns


# ---------------------------------------------------------------------------------------
# Transformer decoder: attention loss (+ auxiliary CTC) as one autograd node over the encoder output
# ---------------------------------------------------------------------------------------
class _AttnDecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, training, eouts, elens_dev, ys_host, ylens_host, ys_in, ys_out, blank, soft, kd, *params):
        logits, st = eng.dec_forward(eouts, elens_dev, ys_in, ylens_host, training, True)
        if soft is None:
            loss_att, _ = eng.att_loss(logits, ys_out, ylens_host)
            loss_kd, loss = torch.zeros_like(loss_att), loss_att
        else:  # label interpolation with the teacher's soft labels (decoders/transformer.py:117-126)
            loss_kd, loss_att, _ = eng.att_kd_loss(logits, ys_out, ylens_host, soft)
            loss = kd * loss_kd + (1 - kd) * loss_att
        loss_ctc, cctx = None, None
        ctx.soft, ctx.kd = soft, kd
        if eng.mtl_ctc > 0:
            ctc_logits = eng.head_logits(eouts, "decoder.ctc.output")
            loss_ctc, cctx = eng.ctc_loss(ctc_logits, elens_dev, ys_host, ylens_host, blank, True)
            loss = loss + eng.mtl_ctc * loss_ctc
        else:
            loss_ctc = torch.zeros_like(loss_att)
        ctx.eng, ctx.st, ctx.cctx, ctx.eouts, ctx.logits = eng, st, cctx, eouts, logits
        ctx.ys_out, ctx.ylens_host = ys_out, ylens_host
        ctx.mark_non_differentiable(logits)
        return loss, loss_att, loss_ctc, logits, loss_kd

    @staticmethod
    def backward(ctx, g_total, g_att, g_ctc, _, g_kd):
        eng = ctx.eng
        if ctx.soft is None:
            g_att_eff = (g_total + g_att).to(torch.float32).reshape(1)
            _, dlogits = eng.att_loss(ctx.logits, ctx.ys_out, ctx.ylens_host, True, g_att_eff)
        else:
            _, _, dlogits = eng.att_kd_loss(ctx.logits, ctx.ys_out, ctx.ylens_host, ctx.soft,
                                            (g_total * ctx.kd + g_kd).to(torch.float32),
                                            (g_total * (1 - ctx.kd) + g_att).to(torch.float32))
        deouts = eng.dec_backward(ctx.st, dlogits)
        if ctx.cctx is not None:
            g_ctc_eff = (g_total * eng.mtl_ctc + g_ctc).to(torch.float32).reshape(1)
            dcl = eng.ctc_grad(ctx.cctx, 1.0, g_ctc_eff)
            from .. import ops
            deouts = ops.add(deouts, eng.head_backward(ctx.eouts, dcl, "decoder.ctc.output"))
        ctx.st = ctx.cctx = ctx.soft = None
        return (None, None, deouts, None, None, None, None, None, None, None, None) + (None,) * len(eng.arena.params)


def attn_decoder_apply(dec, eouts, elens, ys, ylens, ys_in, ys_out, soft_labels=None, kd_weight=0.0):
    eng = _engine_of(dec)
    ylens_host = _host_list(ylens)
    L = max(ylens_host) + 1
    ys_host = ys.cpu() if torch.is_tensor(ys) else torch.as_tensor(ys)
    ys_in = (ys_in.cpu() if torch.is_tensor(ys_in) else torch.as_tensor(ys_in))[:, :L]
    ys_out = (ys_out.cpu() if torch.is_tensor(ys_out) else torch.as_tensor(ys_out))[:, :L]
    soft = None
    if soft_labels is not None:
        soft = torch.as_tensor(soft_labels)[:, :L].to(device=eouts.device, dtype=torch.float32).contiguous()
    return _AttnDecoderFn.apply(eng, dec.training, eouts, _elens_dev(eouts, elens), ys_host, ylens_host, ys_in, ys_out,
                                dec.blank_id, soft, float(kd_weight), *eng.arena.params)


def attn_decoder_logits(dec, eouts, elens, ys_in, ylens):
    eng = _engine_of(dec)
    ys_in = ys_in.cpu() if torch.is_tensor(ys_in) else torch.as_tensor(ys_in)
    cmlm = getattr(dec, "cmlm", False)
    ylens_host = _host_list(ylens) if ylens is not None else [ys_in.shape[1] - (0 if cmlm else 1)] * ys_in.shape[0]
    with torch.no_grad():
        logits, _ = eng.dec_forward(eouts, _elens_dev(eouts, elens), ys_in, ylens_host, dec.training, False, causal=not cmlm)
    return logits


# ---------------------------------------------------------------------------------------
# LAS decoder: attention loss (+ auxiliary CTC) as one autograd node over the encoder output (engine/las.py)
# ---------------------------------------------------------------------------------------
class _LASDecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, training, p_attn, eouts, elens_dev, ys_host, ylens_host, ys_in, ys_out, blank, soft, kd, *params):
        logits, st = eng.las_forward(eouts, elens_dev, ys_in, ylens_host, training, p_attn, True)
        if soft is None:
            loss_att, _ = eng.att_loss(logits, ys_out, ylens_host)
            loss_kd, loss = torch.zeros_like(loss_att), loss_att
        else:  # DistillLoss (las.py:109-116, criteria.py:66-100)
            loss_kd, loss_att, _ = eng.att_kd_loss(logits, ys_out, ylens_host, soft)
            loss = kd * loss_kd + (1 - kd) * loss_att
        loss_ctc, cctx = None, None
        ctx.soft, ctx.kd = soft, kd
        if eng.mtl_ctc > 0:
            ctc_logits = eng.head_logits(eouts, "decoder.ctc.output")
            loss_ctc, cctx = eng.ctc_loss(ctc_logits, elens_dev, ys_host, ylens_host, blank, True)
            loss = loss + eng.mtl_ctc * loss_ctc
        else:
            loss_ctc = torch.zeros_like(loss_att)
        ctx.eng, ctx.st, ctx.cctx, ctx.eouts, ctx.logits = eng, st, cctx, eouts, logits
        ctx.ys_out, ctx.ylens_host = ys_out, ylens_host
        ctx.mark_non_differentiable(logits)
        return loss, loss_att, loss_ctc, logits, loss_kd

    @staticmethod
    def backward(ctx, g_total, g_att, g_ctc, _, g_kd):
        eng = ctx.eng
        if ctx.soft is None:
            g_att_eff = (g_total + g_att).to(torch.float32).reshape(1)
            _, dlogits = eng.att_loss(ctx.logits, ctx.ys_out, ctx.ylens_host, True, g_att_eff)
        else:
            _, _, dlogits = eng.att_kd_loss(ctx.logits, ctx.ys_out, ctx.ylens_host, ctx.soft,
                                            (g_total * ctx.kd + g_kd).to(torch.float32),
                                            (g_total * (1 - ctx.kd) + g_att).to(torch.float32))
        deouts = eng.las_backward(ctx.st, dlogits)
        if ctx.cctx is not None:
            g_ctc_eff = (g_total * eng.mtl_ctc + g_ctc).to(torch.float32).reshape(1)
            dcl = eng.ctc_grad(ctx.cctx, 1.0, g_ctc_eff)
            from .. import ops
            deouts = ops.add(deouts, eng.head_backward(ctx.eouts, dcl, "decoder.ctc.output"))
        ctx.st = ctx.cctx = ctx.soft = None
        return (None, None, None, deouts, None, None, None, None, None, None, None, None) + (None,) * len(eng.arena.params)


def las_decoder_apply(dec, eouts, elens, ys, ylens, ys_in, ys_out, soft_labels=None, kd_weight=0.0):
    """LASDecoder.forward -> (loss, loss_att, loss_ctc, logits [B, L, V], loss_kd); the logits are specified on the positions
    below ylens + 1 of every row (the rest is never read by the loss)"""
    eng = _engine_of(dec)
    ylens_host = _host_list(ylens)
    L = max(ylens_host) + 1
    ys_host = ys.cpu() if torch.is_tensor(ys) else torch.as_tensor(ys)
    ys_in = (ys_in.cpu() if torch.is_tensor(ys_in) else torch.as_tensor(ys_in))[:, :L]
    ys_out = (ys_out.cpu() if torch.is_tensor(ys_out) else torch.as_tensor(ys_out))[:, :L]
    assert 0 <= int(ys_in.min()) and int(ys_in.max()) < dec.vocab_size, "token id outside the vocabulary"
    T = int(max(_host_list(elens)))
    eouts = eouts[:, :T].to(eng.dtype).contiguous()    # frames past the longest utterance carry no weight
    soft = None
    if soft_labels is not None:
        soft = torch.as_tensor(soft_labels)[:, :L].to(device=eouts.device, dtype=torch.float32).contiguous()
    return _LASDecoderFn.apply(eng, dec.training, float(dec.score.dropout_attn_rate), eouts, _elens_dev(eouts, elens), ys_host,
                               ylens_host, ys_in, ys_out, dec.blank_id, soft, float(kd_weight), *eng.arena.params)


def las_beam_apply(dec, eouts, beam_width, len_weight, lm=None, lm_weight=0):
    """LASDecoder.decode's beam search for one utterance -> (hyps, scores); lm with lm_weight > 0: fused on the host form"""
    eng = _engine_of(dec)
    if lm is None or lm_weight <= 0:
        return eng.las_beam_search(eouts, beam_width, len_weight, dec.eos_id, dec.max_decode_ylen)
    return eng.las_beam_search(eouts, beam_width, len_weight, dec.eos_id, dec.max_decode_ylen, lm=lm, lm_weight=lm_weight)


LAS_BATCH_MAX_BEAM = 32   # rows of a search in csrc/las_beam.hip and in emoasr_beam_update_batch
_LAS_FUSION_LOGGED = lockstep._LOGGED   # what log_once has emitted (las_fusion_route, las_fusion_grid_apply)


def las_lm_fusion(dec):
    """the decoder's switch for its LM arguments: "ignore" (default: accepted and not read, as the reference's `pass`) or "fuse";
    anything else is refused"""
    mode = getattr(dec, "las_lm_fusion", "ignore")
    if mode not in ("ignore", "fuse"):
        raise ValueError(f"emoasr_amd: las_lm_fusion is 'ignore' or 'fuse', not {mode!r}")
    return mode


def las_rnnlm_why_not(dec, beam_width, lm):
    """why the batched LAS search cannot fuse this LM through emoasr_rnnlm_step_rows (None: it can):
    lockstep.rnnlm_rows_why_not's reasons, then the beam width"""
    V = dec.vocab_size
    why = lockstep.rnnlm_rows_why_not(_engine_of(dec), V, lm)
    if why is not None:
        return why
    if not 1 <= beam_width <= min(LAS_BATCH_MAX_BEAM, V):
        return f"beam_width {beam_width} (vocabulary {V}) is outside the device bookkeeping's {LAS_BATCH_MAX_BEAM} beams"
    return None


def las_tlm_fusion_of(dec):
    """the decoder's las_tlm_fusion: "host" (the default; a Transformer LM is fused by one host search per utterance, as ever) or
    "device" (stepped inside the batched search over the prefix tree); anything else is a ValueError.  It
    matters only under las_lm_fusion = "fuse" with lm_weight > 0 and a Transformer LM."""
    impl = getattr(dec, "las_tlm_fusion", "host")
    if impl not in ("host", "device"):
        raise ValueError(f"emoasr_amd: las_tlm_fusion is 'host' or 'device', not {impl!r}")
    return impl


def las_tlm_why_not(dec, beam_width, lm):
    """why the batched LAS search cannot step this LM over the prefix tree (None: it can): ctc_tlm_why_not's
    reasons -- a causal Transformer LM in f32 or bf16 (its own compute dtype: the score kernel reads f32 rows either way), its heads
    inside emoasr_lm_tree_attn's plan -- with the LDS bound taken on the search's own longest prefix Lcap = min(max_decode_ylen,
    max_seq_len) and the LM's vocabulary EQUAL to the model's (emoasr_beam_scores_topk soft-maxes the first V columns, the rule
    of the RNN form), then the beam width"""
    from .. import lm_tree
    why = lockstep.lm_type_why_not(lm, "transformer")
    if why is None and not getattr(lm, "causal", False):
        why = "there is no causal LM (the prefix tree steps p(next token | prefix))"
    if why is None and getattr(lm, "compute_dtype", None) not in (torch.float32, torch.bfloat16):
        why = f"the LM computes in {getattr(lm, 'compute_dtype', None)} (emoasr_lm_tree_step takes f32 or bf16)"
    if why is not None:
        return why
    P, V = lm.params, dec.vocab_size
    if P.vocab_size != V:
        return f"the LM's vocabulary ({P.vocab_size}) is not the model's ({V})"
    if not lm_tree.head_ok(P.hidden_size, P.num_attention_heads):
        return (f"the LM's heads ({P.hidden_size} over {P.num_attention_heads}) are outside emoasr_lm_tree_attn's plan "
                f"(8 .. 128 wide, a multiple of 8)")
    Lcap = lm_tree.las_list_cap(dec.max_decode_ylen, P.max_seq_len)
    if lm_tree.attn_lds_bytes(Lcap) > lm_tree.LDS_BYTES:
        return (f"prefixes of {Lcap} tokens need {lm_tree.attn_lds_bytes(Lcap)} bytes of LDS in emoasr_lm_tree_attn "
                f"({lm_tree.LDS_BYTES} at most)")
    if not 1 <= beam_width <= min(LAS_BATCH_MAX_BEAM, V):
        return f"beam_width {beam_width} (vocabulary {V}) is outside the device bookkeeping's {LAS_BATCH_MAX_BEAM} beams"
    return None


def _las_tlm_on_device(dec, lm):
    """a Transformer LM under las_tlm_fusion = "device": the prefix tree's route (the switch is not read for another LM)"""
    return getattr(lm, "lm_type", None) == "transformer" and las_tlm_fusion_of(dec) == "device"


def _las_tlm_require(dec, beam_width, lm):
    why = las_tlm_why_not(dec, beam_width, lm)
    if why is not None:
        raise ValueError(f"emoasr_amd: las_tlm_fusion = 'device' cannot fuse this LM: {why}")


def las_fusion_route(dec, beam_width, lm, lm_weight):
    """-> (lm, lm_weight, why): what LASDecoder.decode's search fuses.  (None, 0, None) under las_lm_fusion == "ignore", without an
    LM or with lm_weight <= 0: today's search.  Under "fuse" a masked LM is refused (require_next_token_lm's messages); why is
    None where the batched device form takes the LM, else las_rnnlm_why_not's reason -- logged once -- and the caller runs the
    host form per utterance.  A Transformer LM under las_tlm_fusion = "device" goes to the prefix tree: why is None, and an LM
    the tree cannot take (las_tlm_why_not) is a ValueError here, before any search."""
    if las_lm_fusion(dec) != "fuse" or lm is None or lm_weight <= 0:
        return None, 0, None
    from .lm import require_next_token_lm
    require_next_token_lm(lm, lm_weight)
    if _las_tlm_on_device(dec, lm):
        _las_tlm_require(dec, beam_width, lm)
        return lm, lm_weight, None
    why = las_rnnlm_why_not(dec, beam_width, lm)
    if why is not None:
        lockstep.log_once(logging.getLogger(__name__), f"LAS beam search: the LM is fused by one host search per utterance: {why}")
    return lm, lm_weight, why


def _las_check_elens(eouts, elens, what):
    elens = [int(n) for n in elens]
    B, T = eouts.shape[0], eouts.shape[1]
    if len(elens) != B or any(n < 1 or n > T for n in elens):
        raise ValueError(f"{what}: every utterance needs 1 <= elens[b] <= {T} frames, got elens {elens}")
    return elens


def las_beam_batch_apply(dec, eouts, elens, beam_width, len_weight, batched=True, lm=None, lm_weight=0):
    """LASDecoder.decode's beam search for every utterance of the batch, utterance b over its own elens[b] frames
    -> (hyps[b], scores[b]).  batched: all utterances in lockstep on the device (engine/las.py:las_beam_search_batch); beams wider
    than 32 or than the vocabulary, and batched=False, run las_beam_search once per utterance.  lm with lm_weight > 0 (already
    routed: las_fusion_route): fused on the device where las_rnnlm_why_not (a Transformer LM under las_tlm_fusion = "device":
    las_tlm_why_not) has no objection, else by the host form per utterance."""
    eng = _engine_of(dec)
    elens = _las_check_elens(eouts, elens, "LASDecoder.decode")
    B = eouts.shape[0]
    fuse = lm is not None and lm_weight > 0
    if batched and 1 <= beam_width <= min(LAS_BATCH_MAX_BEAM, dec.vocab_size):
        if not fuse:
            return eng.las_beam_search_batch(eouts, elens, beam_width, len_weight, dec.eos_id, dec.max_decode_ylen)
        if (las_tlm_why_not if _las_tlm_on_device(dec, lm) else las_rnnlm_why_not)(dec, beam_width, lm) is None:
            return eng.las_beam_search_batch(eouts, elens, beam_width, len_weight, dec.eos_id, dec.max_decode_ylen, lm=lm,
                                             lm_weight=lm_weight)
    hyps, scores = [], []
    for b in range(B):
        h, s = las_beam_apply(dec, eouts[b:b + 1, :elens[b]], beam_width, len_weight, lm if fuse else None, lm_weight if fuse else 0)
        hyps.append(h)
        scores.append(s)
    return hyps, scores


def las_fusion_grid_apply(dec, eouts, elens, beam_width, lm, lm_weights, len_weights):
    """the LAS search of every utterance for every (lm_weight, len_weight) cell -> (hyps[b][cell][n], scores[b][cell][n]), cells in
    lm_weight-outer, len_weight-inner order.  Where the device form takes the LM: ONE
    las_beam_search_batch grid call.  Else (las_rnnlm_why_not's reason, logged once): one host-form search per utterance and
    distinct lm_weight at len_weight 0, the len_weights expanded on the host as the device grid expands them."""
    from .lm import require_next_token_lm
    lm_weights, len_weights = [float(a) for a in lm_weights], [float(b) for b in len_weights]
    eng = _engine_of(dec)
    elens = _las_check_elens(eouts, elens, "las_fusion_grid")
    weights = lockstep.grid_cell_plan(lm_weights, len_weights, lm is not None)[0]
    top = max(weights)
    why = None
    if top > 0:
        require_next_token_lm(lm, top)
        if _las_tlm_on_device(dec, lm):      # the prefix tree (section 33), or a ValueError with its reason
            _las_tlm_require(dec, beam_width, lm)
        else:
            why = las_rnnlm_why_not(dec, beam_width, lm)
    if why is None and 1 <= beam_width <= min(LAS_BATCH_MAX_BEAM, dec.vocab_size):
        return eng.las_beam_search_batch(eouts, elens, beam_width, 0, dec.eos_id, dec.max_decode_ylen, lm=lm if top > 0 else None,
                                         lm_weights=lm_weights, len_weights=len_weights)
    if why is not None:
        lockstep.log_once(logging.getLogger(__name__), f"LAS fusion grid: one host search per utterance and lm_weight: {why}")
    # utterance by utterance, every search weight of one before the next; the driver assembles the cells
    per = [[las_beam_apply(dec, eouts[b:b + 1, :elens[b]], beam_width, 0, lm if a > 0 else None, a) for a in weights]
           for b in range(len(elens))]

    def search_plain():
        k = weights.index(0.0)
        return [p[k][0] for p in per], [p[k][1] for p in per]

    def search_fused(positive, weights, found):
        for b, p in enumerate(per):
            for k in positive:
                found[b][k] = p[k]

    return lockstep.run_fusion_grid(len(elens), lm_weights, len_weights, lm is not None, search_plain, search_fused,
                                    lambda f, a: lockstep.expand_len_weights(*f, len_weights))


class _CMLMDecoderFn(torch.autograd.Function):
    """the conditional masked LM decoder (decoders/transformer.py:102-105,127-128): bidirectional self-attention over ylens keys,
    MaskedLMLoss on the labelled rows"""

    @staticmethod
    def forward(ctx, eng, training, eouts, elens_dev, ys_in, ylens_host, labels, want_logits, *params):
        x, st = eng.dec_forward(eouts, elens_dev, ys_in, ylens_host, training, True, causal=False, head=False)
        B, L = ys_in.shape
        dev = eouts.device
        valid = labels != -100
        count = int(valid.sum())
        # the labelled rows only (no label at all: one row of weight 0, as the BERT LM does)
        rows_host = valid.reshape(-1).nonzero().view(-1) if count else torch.zeros(1, dtype=torch.int64)
        lab = h2d_i32(labels.reshape(-1)[rows_host].clamp(min=0), dev)
        w = torch.full((rows_host.numel(),), 1.0 / count if count else 0.0).pin_memory().to(dev, non_blocking=True)
        sel = rows_host.pin_memory().to(dev, non_blocking=True)
        loss, hst, logits = eng.cmlm_head(x, sel, lab, w, True, want_logits)
        ctx.eng, ctx.st, ctx.hst, ctx.rows = eng, st, hst, B * L
        logits = logits.view(B, L, -1) if logits is not None else eouts.new_empty(0)
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, g, _):
        eng = ctx.eng
        dx = eng.cmlm_head_backward(ctx.hst, ctx.rows, g.to(torch.float32).reshape(1))
        deouts = eng.dec_backward(ctx.st, None, dx=dx)
        ctx.st = ctx.hst = None
        return (None, None, deouts, None, None, None, None, None) + (None,) * len(eng.arena.params)


def cmlm_decoder_apply(dec, eouts, elens, ylens, ys_in, labels, want_logits=False):
    """-> (loss, logits [B, L, V] | an empty tensor)"""
    eng = _engine_of(dec)
    ylens_host = _host_list(ylens)
    L = max(ylens_host)
    ys_in = (ys_in.cpu() if torch.is_tensor(ys_in) else torch.as_tensor(ys_in))[:, :L].to(torch.int64).contiguous()
    labels = (labels.cpu() if torch.is_tensor(labels) else torch.as_tensor(labels))[:, :L].to(torch.int64).contiguous()
    assert labels.shape == ys_in.shape and int(labels.max()) < dec.vocab_size, "labels: [B, L] ids below vocab_size or -100"
    assert 0 <= int(ys_in.min()) and int(ys_in.max()) < dec.vocab_size, "token id outside the vocabulary"
    return _CMLMDecoderFn.apply(eng, dec.training, eouts, _elens_dev(eouts, elens), ys_in, ylens_host, labels, want_logits,
                                *eng.arena.params)


# ---------------------------------------------------------------------------------------
# RNN-T: transducer loss (+ auxiliary CTC) as one autograd node over the encoder output
# ---------------------------------------------------------------------------------------
class _PredNetFn(torch.autograd.Function):
    """the RNN-T prediction network of several micro-batches in one pass (engine.rnnt_prediction_stacked)"""

    @staticmethod
    def forward(ctx, eng, training, ys_in_list, *params):
        douts, rst, spans = eng.rnnt_prediction_stacked(ys_in_list, training)
        ctx.eng, ctx.rst = eng, rst
        ctx.spans = spans
        return douts

    @staticmethod
    def backward(ctx, g):
        from .. import ops
        eng = ctx.eng
        with eng._scope():   # (the engine's own product mode: this runs on an autograd thread)
            eng.arena.attach_grads()
            eng.rnnt_recurrency_bwd(ctx.rst, g.contiguous())
        ctx.rst = None
        return (None, None, None) + (None,) * len(eng.arena.params)


def rnnt_prediction_stacked(dec, ys_in_list, ylens_list):
    """-> one [U_k, B_k, H] prediction-network output per micro-batch (inputs of rnnt_apply(..., pred=...)), all computed in ONE
    pass, or None when the stacked pass does not apply (then every micro-batch runs its own, as before)"""
    eng = _engine_of(dec)
    mats = []
    for ys_in, ylens in zip(ys_in_list, ylens_list):
        L = max(_host_list(ylens))
        mats.append((ys_in.cpu() if torch.is_tensor(ys_in) else torch.as_tensor(ys_in))[:, : L + 1])
    if len(mats) < 2 or not eng.rnnt_prediction_stacked_ok(sum(m.shape[0] for m in mats)):
        return None
    douts = _PredNetFn.apply(eng, dec.training, mats, *eng.arena.params)
    out, b0 = [], 0
    for m in mats:
        out.append(douts[: m.shape[1], b0:b0 + m.shape[0]].contiguous())
        b0 += m.shape[0]
    return out


class _RNNTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, training, eouts, elens_dev, ys_host, ylens_host, ys_in, blank, kd, want_logits, pred, *params):
        """kd = None | (soft f32 [B,L,V] on the device, kd_weight, reduce_main_loss_kd): word-level distillation
        (rnn_transducer.py:127-141, criteria.py:218-247) of every lattice cell towards its label's soft target"""
        from .. import ops
        from ..criteria import rnnt_word_rows
        # the 4-D logits are formed only when something reads them: distillation, or a caller that asked for them
        # (RNNTDecoder.return_logits); training without either runs the fused output layer and returns logits = None
        # with an auxiliary CTC branch the transducer lattice (2 B blocks, ~190 us of a mostly idle chip) runs on a side stream under it
        loss_rnnt, logits, st = eng.rnnt_forward(eouts, elens_dev, ys_in, ys_host, ylens_host, blank, training,
                                                 want_logits=want_logits or kd is not None,
                                                 pred=None if pred is None else pred.detach(),
                                                 defer_lattice=eng.mtl_ctc > 0)
        cctx, loss = None, loss_rnnt
        if eng.mtl_ctc > 0:
            ctc_logits = eng.head_logits(eouts, "decoder.ctc.output")
            loss_ctc, cctx = eng.ctc_loss(ctc_logits, elens_dev, ys_host, ylens_host, blank, True)
            if loss_rnnt is None:
                loss_rnnt = eng.rnnt_lattice_join(st)
            loss = loss_rnnt + eng.mtl_ctc * loss_ctc
        else:
            loss_ctc = torch.zeros_like(loss_rnnt)
        loss_kd = torch.zeros_like(loss_rnnt)
        ctx.kd = None
        if kd is not None:
            soft, kd_w, reduce, kd_type = kd
            B, T, U, V = logits.shape
            L = soft.shape[1]
            if kd_type == "word":
                src, w = rnnt_word_rows(B, T, U, L, elens_dev, ylens_host, logits.device)
                z, lrow = logits.view(B * T * U, V), None
            else:
                # "align" (rnn_transducer.py:131-135): forced alignment from the loss lattices, then
                # RNNTAlignDistillLoss -- whose loop keeps only the LAST label of each utterance
                # (criteria.py:271-281), i.e. one lattice cell per utterance
                alpha, beta = st.ctx[3], st.ctx[4]
                aligns = ops.rnnt_best_path(alpha, beta, st.elens, st.ylens)
                bi = torch.arange(B, device=logits.device, dtype=torch.int32)
                u = (st.ylens - 1).clamp(min=0)
                t = aligns.gather(1, u.long()[:, None].clamp(max=max(aligns.shape[1] - 1, 0)))[:, 0]
                lrow = ((bi * T + t) * U + u).long()
                z = logits.view(B * T * U, V).index_select(0, lrow)  # [B,V], kept: the logits get overwritten
                src = (bi * L + u).to(torch.int32)
                w = (1.0 / B) / st.ylens.clamp(min=1).to(torch.float32)
            rows, _ = ops.soft_ce(z, soft.view(B * L, V), src, None, w, None, 0.0)
            loss_kd = rows.sum()
            loss = ((1 - kd_w) * loss if reduce else loss) + kd_w * loss_kd
            ctx.kd = (soft, kd_w, (1 - kd_w) if reduce else 1.0, src, w, z, lrow)
        ctx.eng, ctx.st, ctx.cctx, ctx.eouts = eng, st, cctx, eouts
        if logits is None:
            logits = eouts.new_empty(0)   # (autograd outputs must be tensors; rnnt_apply turns it back into None)
        ctx.mark_non_differentiable(logits)
        return loss, loss_rnnt, loss_ctc, logits, loss_kd

    @staticmethod
    def backward(ctx, g_total, g_rnnt, g_ctc, _, g_kd):
        from .. import ops
        eng = ctx.eng
        main, extra = 1.0, None
        if ctx.kd is not None:  # before rnnt_backward overwrites the logits with their gradient
            soft, kd_w, main, src, w, z, lrow = ctx.kd
            V = z.shape[-1]
            _, extra = ops.soft_ce(z, soft.view(-1, V), src, None, w * (g_total * kd_w + g_kd).to(torch.float32), None,
                                   0.0, want_grad=True)
            extra = extra if lrow is None else (lrow, extra)
        deouts = eng.rnnt_backward(ctx.st, (g_total * main + g_rnnt).to(torch.float32).reshape(1), extra)
        if ctx.cctx is not None:
            g_ctc_eff = (g_total * (main * eng.mtl_ctc) + g_ctc).to(torch.float32).reshape(1)
            dcl = eng.ctc_grad(ctx.cctx, 1.0, g_ctc_eff)
            deouts = ops.add(deouts, eng.head_backward(ctx.eouts, dcl, "decoder.ctc.output"))
        dpred = getattr(ctx.st, "ddouts", None)   # (the prediction network ran stacked: its gradient goes back to that pass)
        ctx.st = ctx.cctx = ctx.kd = None
        return (None, None, deouts, None, None, None, None, None, None, None, dpred) + (None,) * len(eng.arena.params)


def rnnt_apply(dec, eouts, elens, ys, ylens, ys_in, kd=None, pred=None):
    eng = _engine_of(dec)
    ylens_host = _host_list(ylens)
    L = max(ylens_host)
    ys_host = (ys.cpu() if torch.is_tensor(ys) else torch.as_tensor(ys))[:, :L]
    ys_in = (ys_in.cpu() if torch.is_tensor(ys_in) else torch.as_tensor(ys_in))[:, : L + 1]
    if kd is not None:
        kd = (torch.as_tensor(kd[0]).to(device=eouts.device, dtype=torch.float32).contiguous(), float(kd[1]), bool(kd[2]),
              kd[3])
    want_logits = bool(getattr(dec, "return_logits", False)) or not dec.training
    out = _RNNTFn.apply(eng, dec.training, eouts, _elens_dev(eouts, elens), ys_host, ylens_host, ys_in, dec.blank_id, kd,
                        want_logits, pred, *eng.arena.params)
    loss, loss_rnnt, loss_ctc, logits, loss_kd = out
    return loss, loss_rnnt, loss_ctc, (logits if logits.numel() else None), loss_kd


def rnnt_forced_align_apply(log_probs, elens, ys, ylens, blank):
    """RNNTForcedAligner.__call__ (rnnt_aligner.py:158-198) -> int32 [B,L] (device)"""
    from .. import ops
    dev = log_probs.device
    z = log_probs.contiguous()
    B, T, U, V = z.shape
    labels = torch.as_tensor(ys)[:, : max(U - 1, 1)].to(torch.int32)
    if labels.shape[1] < max(U - 1, 1):
        labels = torch.nn.functional.pad(labels, (0, max(U - 1, 1) - labels.shape[1]))
    labels = labels.contiguous().to(dev)
    el = torch.as_tensor(elens).to(torch.int32).to(dev)
    yl = torch.as_tensor(ylens).to(torch.int32).to(dev)
    with ops.stream_scope():
        (_, _, _, alpha, beta), _ = ops.rnnt_forward(z, labels, el, yl, blank)
        return ops.rnnt_best_path(alpha, beta, el, yl)


def rnnt_greedy_apply(dec, eouts, elens):
    """dec.rnnt_greedy_impl: "utterance" (one search per utterance, engine.rnnt_greedy) or "batch" (all utterances in lockstep,
    engine.rnnt_greedy_batch; a model that form cannot take is a ValueError naming the reason -- no quiet detour)"""
    impl = getattr(dec, "rnnt_greedy_impl", "utterance")
    if impl not in ("utterance", "batch"):
        raise ValueError(f"emoasr_amd: rnnt_greedy_impl is 'utterance' or 'batch', not {impl!r}")
    eng = _engine_of(dec)
    if impl == "batch":    # (the engine refuses a model it cannot take: rnnt_greedy_batch_why_not)
        return eng.rnnt_greedy_batch(eouts, _host_list(elens), dec.blank_id, dec.eos_id, dec.max_seq_len)
    return eng.rnnt_greedy(eouts, _host_list(elens), dec.blank_id, dec.eos_id, dec.max_seq_len)


def rnnt_beam_apply(dec, eouts, beam_width, lm=None, lm_weight=0, len_weight=0):
    return _engine_of(dec).rnnt_beam_search(eouts, beam_width, dec.blank_id, dec.eos_id, lm=lm, lm_weight=lm_weight,
                                            len_weight=len_weight)


def rnnt_tlm_fusion_of(dec):
    """the decoder's rnnt_tlm_fusion: "host" (the default; a Transformer LM is fused utterance by utterance on the host, as ever) or
    "device" (fused on the device over the prefix tree); anything else is a ValueError"""
    impl = getattr(dec, "rnnt_tlm_fusion", "host")
    if impl not in ("host", "device"):
        raise ValueError(f"emoasr_amd: rnnt_tlm_fusion is 'host' or 'device', not {impl!r}")
    return impl


def ctc_tlm_fusion_of(dec):
    """the decoder's ctc_tlm_fusion: "host" (the default; the fused CTC search scores a Transformer LM's new prefixes with one
    lm.predict per frame, as ever) or "device" (stepped on the device over the prefix tree); anything else is
    a ValueError.  It matters only under ctc_beam_impl = "device" with lm_weight > 0 and a causal Transformer LM."""
    impl = getattr(dec, "ctc_tlm_fusion", "host")
    if impl not in ("host", "device"):
        raise ValueError(f"emoasr_amd: ctc_tlm_fusion is 'host' or 'device', not {impl!r}")
    return impl


def ctc_tlm_why_not(dec, lm):
    """why the fused CTC search cannot step this LM over the prefix tree (None: it can): a causal Transformer
    LM in f32 or bf16 (its own compute dtype: the pool rows are f32 either way), its vocabulary at least the CTC head's, its heads
    and its longest prefix inside emoasr_lm_tree_attn's plan"""
    from .. import lm_tree, lockstep
    why = lockstep.lm_type_why_not(lm, "transformer")
    if why is None and not getattr(lm, "causal", False):
        why = "there is no causal LM (the prefix tree steps p(next token | prefix))"
    if why is None and getattr(lm, "compute_dtype", None) not in (torch.float32, torch.bfloat16):
        why = f"the LM computes in {getattr(lm, 'compute_dtype', None)} (emoasr_lm_tree_step takes f32 or bf16)"
    if why is not None:
        return why
    P = lm.params
    if P.vocab_size < dec.vocab_size:
        return f"the LM's vocabulary ({P.vocab_size}) is smaller than the model's ({dec.vocab_size})"
    if not lm_tree.head_ok(P.hidden_size, P.num_attention_heads):
        return (f"the LM's heads ({P.hidden_size} over {P.num_attention_heads}) are outside emoasr_lm_tree_attn's plan "
                f"(8 .. 128 wide, a multiple of 8)")
    if lm_tree.attn_lds_bytes(P.max_seq_len) > lm_tree.LDS_BYTES:
        return (f"max_seq_len {P.max_seq_len} needs {lm_tree.attn_lds_bytes(P.max_seq_len)} bytes of LDS in emoasr_lm_tree_attn "
                f"({lm_tree.LDS_BYTES} at most)")
    return None


def rnnt_beam_batch_apply(dec, eouts, elens, beam_width, lm=None, lm_weights=None, len_weights=None, require_device=False,
                          tlm_fusion="host"):
    """-> (hyps[b][n], scores[b][n]): every utterance searched over its own elens[b] frames; with lm_weights the shallow-fusion
    grid (hyps[b][cell][n], scores[b][cell][n]: engine.rnnt_beam_search_batch).  require_device: a ValueError naming the reason
    where the device form cannot fuse this LM, instead of the host form.  tlm_fusion = "device": a Transformer LM is fused on the
    device over the prefix tree (the engine refuses, by name, an LM that form cannot take)"""
    if tlm_fusion not in ("host", "device"):
        raise ValueError(f"emoasr_amd: rnnt_tlm_fusion is 'host' or 'device', not {tlm_fusion!r}")
    eng = _engine_of(dec)
    tlm = tlm_fusion == "device" and getattr(lm, "lm_type", None) == "transformer"
    if require_device and not tlm and lm is not None and lm_weights is not None and any(float(a) > 0 for a in lm_weights):
        why = eng.rnnt_beam_lm_why_not(lm)
        if why is not None:
            raise ValueError(f"emoasr_amd: rnnt_beam_impl = 'device' cannot fuse this LM: {why}")
    if tlm_fusion == "host":      # today's call, unchanged
        return eng.rnnt_beam_search_batch(eouts, _host_list(elens), beam_width, dec.blank_id, dec.eos_id, lm=lm, lm_weights=lm_weights,
                                          len_weights=len_weights)
    return eng.rnnt_beam_search_batch(eouts, _host_list(elens), beam_width, dec.blank_id, dec.eos_id, lm=lm, lm_weights=lm_weights,
                                      len_weights=len_weights, tlm_fusion=tlm_fusion)


def rnnt_fusion_grid_apply(dec, eouts, elens, beam_width, lm, lm_weights, len_weights, tlm_fusion="host"):
    """the transducer search of every utterance for every (lm_weight, len_weight) cell -> (hyps[b][cell][n], scores[b][cell][n]),
    cells in lm_weight-outer, len_weight-inner order"""
    return rnnt_beam_batch_apply(dec, eouts, elens, beam_width, lm, [float(a) for a in lm_weights], [float(b) for b in len_weights],
                                 tlm_fusion=tlm_fusion)
