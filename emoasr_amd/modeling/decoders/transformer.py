"""TransformerDecoder -- module API of asr/modeling/decoders/transformer.py:24-294 on the HIP engine.

    decoder(eouts, elens, eouts_inter, ys, ylens, ys_in, ys_out) -> (loss, loss_dict, logits)
    decoder(eouts, elens, ..., ys_in=ys_in, ys_out=None)         -> logits
    decoder.decode(eouts, elens, eouts_inter, beam_width, len_weight, lm, lm_weight, decode_ctc_weight)

Shallow fusion with a stateful LM (the RNN LM, lm_type "rnn") in the batched search -- several utterances, or one under
joint_beam_impl = "batch" -- follows decoder.joint_rnnlm_impl:
    "host"    (default) one joint_beam_search per utterance with the host bookkeeping: one lm.step, a few device-to-host copies and
              a Python sort per output step and utterance;
    "device"  the LM is stepped inside the captured chain of the batched device search (emoasr_rnnlm_step_rows over all S * W rows,
              its state in slot pools addressed by the chain's own parent array); joint_beam_search_device_grid then searches every
              distinct lm_weight of a fusion grid in one pass.  A configuration this form cannot take -- beam_search_device.
              batch_rnnlm_why_not: another vocabulary or compute dtype than the model's, sizes outside the step kernel's plan, more than
              32 beams or candidates, the switches that force the host bookkeeping -- is a ValueError naming the reason, never a quiet
              detour through the host form.
A Transformer LM is not touched by the switch.  Any other value is a ValueError.
"""
import torch.nn as nn

from ..blocks import TransformerDecoderLayer
from ..functions import attn_decoder_apply, attn_decoder_logits, cmlm_decoder_apply
from .ctc import CTCDecoder


class TransformerDecoder(nn.Module):
    def __init__(self, params, cmlm=False):
        super().__init__()
        self.cmlm = cmlm      # conditional masked LM: bidirectional self-attention, MaskedLMLoss on the labelled positions
        self.vocab_size = params.vocab_size
        self.embed = nn.Embedding(self.vocab_size, params.dec_hidden_size)
        self.dec_num_layers = params.dec_num_layers
        self.transformers = nn.ModuleList(
            TransformerDecoderLayer(params.dec_num_attention_heads, params.dec_hidden_size, params.dec_intermediate_size)
            for _ in range(self.dec_num_layers))
        self.mtl_ctc_weight = params.mtl_ctc_weight
        if self.mtl_ctc_weight > 0:
            self.ctc = CTCDecoder(params, prefix="decoder.ctc")
        self.norm = nn.LayerNorm(params.dec_hidden_size, eps=1e-12)
        self.output = nn.Linear(params.dec_hidden_size, self.vocab_size)
        self.kd_weight = params.kd_weight
        self.blank_id = params.blank_id
        self.eos_id = params.eos_id
        self.max_decode_ylen = params.max_decode_ylen
        # the joint search of ONE utterance: "single" (joint_beam_search) or "batch" (the batched device search with one search in it;
        # DESIGN.md section 21).  Several utterances always take the batched search.
        self.joint_beam_impl = "single"
        # a stateful LM (the RNN LM) in the batched searches: "host" (one single search per utterance) or "device" (stepped inside the
        # batched device search; see the module docstring).  A plain attribute: not a parameter, not saved.
        self.joint_rnnlm_impl = "host"
        self._owner = None

    def forward(self, eouts, elens, eouts_inter=None, ys=None, ylens=None, ys_in=None, ys_out=None,
                soft_labels=None, ps=None, plens=None):
        if ys_out is None:
            return attn_decoder_logits(self, eouts, elens, ys_in, ylens)
        if self.cmlm:
            want = bool(getattr(self._owner[0], "return_logits", False)) if self._owner else False
            loss, logits = cmlm_decoder_apply(self, eouts, elens, ylens, ys_in, ys_out, want)
            return loss, {"loss_att": loss, "loss_total": loss}, logits
        kd = self.kd_weight > 0 and soft_labels is not None  # DistillLoss replaces the label-smoothing loss (:71-79)
        loss, loss_att, loss_ctc, logits, loss_kd = attn_decoder_apply(self, eouts, elens, ys, ylens, ys_in, ys_out,
                                                                       soft_labels if kd else None, self.kd_weight)
        loss_dict = {"loss_kd": loss_kd, "loss_att": loss_att} if kd else {"loss_att": loss_att}
        if self.mtl_ctc_weight > 0:
            loss_dict["loss_ctc"] = loss_ctc
        loss_dict["loss_total"] = loss
        return loss, loss_dict, logits

    def decode(self, eouts, elens, eouts_inter=None, beam_width=1, len_weight=0, lm=None, lm_weight=0,
               decode_ctc_weight=0, decode_phone=False):
        if decode_ctc_weight == 1:
            self.ctc._owner = self._owner
            return self.ctc.decode(eouts, elens, beam_width=1)
        from .. import beam_search as bs
        if self.joint_beam_impl not in ("single", "batch"):
            raise ValueError(f"joint_beam_impl {self.joint_beam_impl!r}: 'single' or 'batch'")
        if self.joint_rnnlm_impl not in ("host", "device"):
            raise ValueError(f"emoasr_amd: joint_rnnlm_impl is 'host' or 'device', not {self.joint_rnnlm_impl!r}")
        B = eouts.shape[0]
        if B == 1 and self.joint_beam_impl == "single":
            return bs.joint_beam_search(self, eouts, elens, beam_width, len_weight, lm, lm_weight, decode_ctc_weight)
        # a batch: N-best lists per utterance (one utterance through "batch": that utterance's lists, the single search's return shape)
        hyps, scores, _, _ = bs.joint_beam_search_batch(self, eouts, elens, beam_width, len_weight, lm, lm_weight, decode_ctc_weight)
        if B == 1:
            return hyps[0], scores[0], None, None
        if beam_width == 1:   # what decode.test_step_batch expects of a greedy batch: one hypothesis (or none) per utterance
            return [h[0] if h else [] for h in hyps], [s[0] if s else None for s in scores], None, None
        return hyps, scores, None, None
