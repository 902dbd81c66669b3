"""LASDecoder -- module API of asr/modeling/decoders/las.py:22-343 (Listen-Attend-Spell: LSTM cells with location-aware additive
attention) on the HIP engine.

    decoder(eouts, elens, eouts_inter, ys, ylens, ys_in, ys_out, soft_labels) -> (loss, loss_dict, logits [B, L, V])
    decoder.decode(eouts, elens, eouts_inter, beam_width, len_weight, ...)    -> (hyps, scores, None, None)

The sub-modules carry the reference's names (nn.LSTMCell `rnns`, `score.w_key / w_query / w_conv / w_score / conv`, `intermed`,
`output`, `ctc.output`), so its checkpoints load; they hold parameters only, the arithmetic runs in engine/las.py and
csrc/las.hip.  As in the reference, the attention weights are dropped with p = 0.1 in train mode -- AttentionLoc's constructor
default, which LASDecoder never overrides and no config field reaches (`decoder.score.dropout_attn_rate` is the attribute).

decode(): `decode_ctc_weight == 1` is CTC greedy; otherwise the reference's beam search (las.py:176-287).  The reference's
intermediate `decode_ctc_weight` branch is `pass`: the value is accepted and ignored here too.  A search that never emits <eos>
returns ([], [], None, None).  The reference takes one utterance; here a batch of several returns (hyps[b], scores[b], None, None),
utterance b searched over its own elens[b] frames -- N-best lists at every beam width, beam 1 included (one-element lists; [] / []
for a search that never ends).  `las_beam_impl`: "single" searches one utterance with the host bookkeeping
(engine/las.py:las_beam_search) and a batch with the lockstep device search (las_beam_search_batch); "batch"
sends one utterance there too.

`lm` / `lm_weight` and the switch `las_lm_fusion`.  The reference's LM branch is `if lm_weight > 0: pass`
(las.py:233): under the default "ignore" the arguments are accepted and their values not read, the search is the reference's bit for
bit.  Under "fuse", with an LM and lm_weight > 0, the LM is fused the way the reference's own attention search fuses it at
decode_ctc_weight == 0 (decoders/transformer.py:217-226, 246-286): the row of a live hypothesis is log_softmax(head)[v] + lm_weight *
log_softmax(LM logits)[v] for v < V, its top beam_width are the expansions, the LM's input is the hypothesis's last token (<eos> at
step 0) and its state follows the parent; a finished hypothesis gains len_weight * len(hyp) as before.  Routes under "fuse":
    several utterances, or one under las_beam_impl == "batch"   the device form: the RNN LM stepped inside the captured chain
    one utterance under "single"                                the host form: any next-token LM, the Transformer LM included
    a Transformer LM under las_tlm_fusion = "device"            the device form over the prefix tree of csrc/lm_tree.hip (DESIGN.md
        (default "host": the row below)                         section 33), for several utterances and for one under "batch"; an
                                                                LM the tree cannot take (functions.las_tlm_why_not: not causal,
                                                                not f32 / bf16, lm V != V, heads or prefix length outside
                                                                emoasr_lm_tree_attn's plan, beam_width > 32 or > V) is a
                                                                ValueError with the reason, before any search
    an LM the device form cannot take (functions.las_rnnlm_why_not: not lm_type "rnn", lm.V != V, another compute dtype or product
        mode, sizes outside emoasr_rnnlm_step_rows' plan), beam_width > 32 or > V
                                                                one host-form search per utterance, the reason logged once,
                                                                the same return shape
    a masked LM (BERT, ELECTRA, P2W, P-ELECTRA)                 refused with lm.require_next_token_lm's messages
lm_weight <= 0 or lm None under "fuse" is the unfused search.

Supported sizes (16-byte accesses): embedding_size, enc_hidden_size, dec_hidden_size, attn_dim and dec_intermediate_size are
multiples of 8, attn_dim <= 512 (one 8-channel group per lane of the attention kernel); batch and lengths are free.
"""
import torch.nn as nn

from ..functions import las_beam_apply, las_beam_batch_apply, las_decoder_apply, las_fusion_route
from .ctc import CTCDecoder

LAS_FIELDS = ("vocab_size", "embedding_size", "enc_hidden_size", "dec_hidden_size", "dec_num_layers", "attn_dim",
              "dec_intermediate_size", "dropout_dec_rate", "lsm_prob", "loss_normalize_length", "loss_normalize_batch", "kd_weight",
              "mtl_ctc_weight", "eos_id", "max_decode_ylen")
LAS_MAX_ATTN_DIM = 512


class AttentionLoc(nn.Module):
    """parameter holder of las.py:289-309 (the step itself is emoasr_las_attend_fwd / _bwd)"""

    def __init__(self, key_dim, query_dim, attn_dim, conv_out_channels=10, conv_kernel_size=201, dropout_attn_rate=0.1):
        super().__init__()
        assert conv_out_channels == 10 and conv_kernel_size == 201, "the attention kernels are built for 10 filters of width 201"
        self.w_key = nn.Linear(key_dim, attn_dim)
        self.w_query = nn.Linear(query_dim, attn_dim)
        self.w_conv = nn.Linear(conv_out_channels, attn_dim)
        self.w_score = nn.Linear(attn_dim, 1)
        self.conv = nn.Conv1d(in_channels=1, out_channels=conv_out_channels, kernel_size=conv_kernel_size, stride=1,
                              padding=(conv_kernel_size - 1) // 2, bias=False)
        self.dropout_attn_rate = dropout_attn_rate

    def forward(self, *args, **kwargs):
        raise RuntimeError("emoasr_amd: AttentionLoc holds parameters; the attention step runs inside LASDecoder on the HIP engine")


class LASDecoder(nn.Module):
    batch_nbest_lists = True   # decode() of a batch returns a LIST of hypotheses per utterance at beam width 1 too (decode.py)

    def __init__(self, params, phase="train"):
        super().__init__()
        for f in LAS_FIELDS:
            if not hasattr(params, f):
                raise AttributeError(f"emoasr_amd: decoder_type='las' needs the config field {f!r}")
        for f in ("embedding_size", "enc_hidden_size", "dec_hidden_size", "attn_dim", "dec_intermediate_size"):
            if int(getattr(params, f)) % 8 != 0:
                raise NotImplementedError(f"emoasr_amd: decoder_type='las' needs {f} to be a multiple of 8 (got {getattr(params, f)})")
        if params.attn_dim > LAS_MAX_ATTN_DIM:
            raise NotImplementedError(f"emoasr_amd: decoder_type='las' needs attn_dim <= {LAS_MAX_ATTN_DIM} (got {params.attn_dim})")
        if params.dec_num_layers < 1:
            raise NotImplementedError("emoasr_amd: decoder_type='las' needs dec_num_layers >= 1")
        self.vocab_size = params.vocab_size
        self.enc_hidden_size = params.enc_hidden_size
        self.dec_hidden_size = params.dec_hidden_size
        self.dec_num_layers = params.dec_num_layers
        self.mtl_ctc_weight = params.mtl_ctc_weight
        if self.mtl_ctc_weight > 0:
            self.ctc = CTCDecoder(params, prefix="decoder.ctc")
        self.embed = nn.Embedding(params.vocab_size, params.embedding_size)
        self.rnns = nn.ModuleList()
        nin = params.embedding_size + params.enc_hidden_size
        for _ in range(self.dec_num_layers):
            self.rnns.append(nn.LSTMCell(nin, params.dec_hidden_size))
            nin = params.dec_hidden_size
        self.score = AttentionLoc(key_dim=params.enc_hidden_size, query_dim=params.dec_hidden_size, attn_dim=params.attn_dim)
        self.intermed = nn.Linear(params.enc_hidden_size + params.dec_hidden_size, params.dec_intermediate_size)
        self.output = nn.Linear(params.dec_intermediate_size, params.vocab_size)
        self.kd_weight = params.kd_weight
        self.blank_id = getattr(params, "blank_id", 0)
        self.eos_id = params.eos_id
        self.max_decode_ylen = params.max_decode_ylen
        self.las_beam_impl = "single"   # "batch": one utterance goes through the batched device search too
        self.las_lm_fusion = "ignore"   # "fuse": decode() fuses its lm / lm_weight arguments (the reference's branch is `pass`)
        self.las_tlm_fusion = "host"    # "device": under "fuse", a Transformer LM is stepped inside the batched search (section 33)
        self._owner = None

    def forward(self, eouts, elens, eouts_inter=None, ys=None, ylens=None, ys_in=None, ys_out=None, soft_labels=None,
                ps=None, plens=None):
        kd = self.kd_weight > 0 and soft_labels is not None   # DistillLoss in place of the label-smoothing loss (las.py:109-120)
        loss, loss_att, loss_ctc, logits, loss_kd = las_decoder_apply(self, eouts, elens, ys, ylens, ys_in, ys_out,
                                                                      soft_labels if kd else None, self.kd_weight)
        loss_dict = {"loss_kd": loss_kd, "loss_att": loss_att} if kd else {"loss_att": loss_att}
        if self.mtl_ctc_weight > 0:
            loss_dict["loss_ctc"] = loss_ctc
        loss_dict["loss_total"] = loss
        return loss, loss_dict, logits

    def decode(self, eouts, elens, eouts_inter=None, beam_width=1, len_weight=0, lm=None, lm_weight=0, decode_ctc_weight=0,
               decode_phone=False):
        if decode_ctc_weight == 1:
            self.ctc._owner = self._owner
            return self.ctc.decode(eouts, elens, beam_width=1)
        if self.las_beam_impl not in ("single", "batch"):
            raise ValueError(f"las_beam_impl {self.las_beam_impl!r}: 'single' or 'batch'")
        lm, lm_weight, _ = las_fusion_route(self, beam_width, lm, lm_weight)     # (None, 0, None) unless las_lm_fusion == "fuse"
        if eouts.size(0) == 1 and self.las_beam_impl == "single":   # las.py:196: the reference's one utterance, all its frames
            hyps, scores = las_beam_apply(self, eouts, beam_width, len_weight, lm, lm_weight)
            return hyps, scores, None, None
        hyps, scores = las_beam_batch_apply(self, eouts, elens, beam_width, len_weight, lm=lm, lm_weight=lm_weight)
        if eouts.size(0) == 1:   # one utterance through "batch": the single search's return shape
            return hyps[0], scores[0], None, None
        return hyps, scores, None, None
