"""P2W -- the phone-to-word models of lm/modeling/p2w.py:20-107 on the HIP engine.

    lm = P2W(params).cuda()                      # params.lm_type: "pbert" | "pctc"
    loss, loss_dict = lm(ys, ylens, labels, ps, plens)     # loss.backward() works
    logits = lm(ys, ylens, ps=ps, plens=plens)             # pbert: [B, L, V]
    hyps = lm.decode(ps, plens)                            # pctc: greedy

A Transformer encoder over phone ids (input_layer "embed", absolute positions) feeds either the conditional masked LM decoder
("pbert": TransformerDecoder(cmlm=True) -- bidirectional self-attention, source attention over the phones, cross-entropy on the masked
positions) or a CTC head ("pctc").  State-dict keys and shapes are the reference's, so its checkpoints load.  P2W owns one engine and
one parameter arena, like ASR; the engine's configuration keys a P2W yaml does not carry (encoder_type, decoder_type,
pos_encode_type) come from a view over the parameters, not from the user.
"""
import logging

import torch
import torch.nn as nn

from .. import ops
from .asr import F32X3
from .decoders.ctc import CTCDecoder
from .decoders.transformer import TransformerDecoder
from .encoders.transformer import TransformerEncoder


class _EngineParams:
    """the user's parameters with the keys the engine reads and a P2W configuration does not contain"""

    def __init__(self, params, **extra):
        self.__dict__["_params"], self.__dict__["_extra"] = params, extra

    def __getattr__(self, key):
        extra = self.__dict__["_extra"]
        if key in extra:
            return extra[key]
        return getattr(self.__dict__["_params"], key)


class P2W(nn.Module):
    def __init__(self, params, phase="train", encoder_type=None, decoder_type=None, return_logits=False,
                 compute_dtype=torch.bfloat16):
        super().__init__()
        self.lm_type = params.lm_type
        logging.info(f"LM type: {self.lm_type}")
        if decoder_type is None:
            decoder_type = {"ptransformer": "transformer", "pbert": "bert", "pctc": "ctc"}.get(self.lm_type)
        if decoder_type not in ("bert", "ctc"):
            raise NotImplementedError(f"emoasr_amd: lm_type={self.lm_type!r} (decoder_type={decoder_type!r}) is outside the HIP hot path")
        if encoder_type not in (None, "transformer"):
            raise NotImplementedError(f"emoasr_amd: P2W with encoder_type={encoder_type!r} is outside the HIP hot path")
        self.decoder_type = decoder_type
        self.params = params
        self.compute_dtype = compute_dtype
        self.encoder = TransformerEncoder(params)
        self.decoder = TransformerDecoder(params, cmlm=True) if decoder_type == "bert" else CTCDecoder(params)
        self.vocab_size = params.vocab_size
        self.eos_id = params.eos_id
        self.add_sos_eos = params.add_sos_eos
        self.return_logits = return_logits
        self._engine_params = _EngineParams(params, encoder_type="transformer", pos_encode_type="abs",
                                            decoder_type="transformer" if decoder_type == "bert" else "ctc")
        self.encoder._owner = [self]
        self.decoder._owner = [self]
        self._engine = None
        n = sum(p.numel() for p in self.parameters())
        logging.info(f"P2W model #parameters: {n} ({sum(p.numel() for p in self.parameters() if p.requires_grad)} trainable)")

    @property
    def compute_dtype(self):
        return self._compute_dtype

    @compute_dtype.setter
    def compute_dtype(self, value):
        split = isinstance(value, str) and value == F32X3
        assert split or value in (torch.float32, torch.bfloat16), f"compute_dtype={value!r}: torch.bfloat16, torch.float32 or 'f32x3'"
        object.__setattr__(self, "f32_split", split)
        object.__setattr__(self, "_compute_dtype", torch.float32 if split else value)

    def engine(self):
        from ..engine import CTCEngine
        if self._engine is None or self._engine.dtype != self.compute_dtype or self._engine.split != self.f32_split:
            self._engine = CTCEngine(self._engine_params, self, self.compute_dtype, f32_split=self.f32_split)
        self._engine._apply_mode()
        return self._engine

    @staticmethod
    def _trim(x, lens):
        if lens is None:
            return x, [int(x.shape[1])] * int(x.shape[0])     # one full-length sequence per row
        lens = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
        return x[:, : max(lens)], lens

    def forward(self, ys=None, ylens=None, labels=None, ps=None, plens=None):
        ps, plens = self._trim(ps, plens)
        ys, ylens = self._trim(ys, ylens)
        if self.decoder_type == "ctc":
            eouts, elens, _ = self.encoder(ps, plens)
            loss, loss_dict, _ = self.decoder(eouts, elens, ys=ys, ylens=ylens)
            return loss, loss_dict
        if labels is None:
            with torch.no_grad():
                eouts, elens, _ = self.encoder(ps, plens)
                return self.decoder(eouts, elens, ys=ys, ylens=ylens, ys_in=ys)
        eouts, elens, _ = self.encoder(ps, plens)
        labels = labels[:, : max(ylens)]
        loss, loss_dict, logits = self.decoder(eouts, elens, ys=ys, ylens=ylens, ys_in=ys, ys_out=labels)
        if self.return_logits:
            return loss, loss_dict, logits
        return loss, loss_dict

    def logits_at(self, ys, ylens, rows, ps, plens):
        """lm_type "pbert", inputs that already lie on the device: ps int [B, Pw] (device) with plens [B] (host, each >= 1); ys int
        [S, Lw] (device), S a multiple of B, sequence s over the phones of utterance s % B; ylens [S] (host, each >= 1); rows int
        [n] (device): flat positions s * Lw + j of ys -> logits [n, V] (compute dtype) of those positions.  The phone encoder runs
        ONCE over the B utterances and its output is indexed per sequence; the decoder stack runs on all tokens, in chunks of
        LM.MAX_TOKEN_ROWS token rows; the final LayerNorm and the vocabulary product run on the n gathered rows alone (the row
        selection of engine.cmlm_head).  Nothing is copied to the host."""
        from .lm import LM
        if self.decoder_type != "bert":
            raise NotImplementedError("emoasr_amd: P2W.logits_at needs the masked-LM decoder (lm_type='pbert')")
        assert ys.is_cuda and rows.is_cuda and ps.is_cuda and ys.dim() == 2 and ps.dim() == 2, "logits_at takes device tensors"
        B, S, Lw = ps.shape[0], ys.shape[0], ys.shape[1]
        yl = [int(v) for v in (ylens.tolist() if torch.is_tensor(ylens) else ylens)]
        pl = [int(v) for v in (plens.tolist() if torch.is_tensor(plens) else plens)]
        assert S % B == 0 and len(yl) == S and len(pl) == B, "ys: a whole number of copies of the batch"
        assert min(yl) >= 1 and max(yl) <= Lw and min(pl) >= 1 and max(pl) <= ps.shape[1], "ylens in [1, Lw], plens in [1, Pw]"
        L, n = max(yl), rows.numel()
        eng = self.engine()
        with torch.no_grad():
            if n == 0:
                return torch.empty(0, self.vocab_size, device=ys.device, dtype=self.compute_dtype)
            eouts, _, elens_dev, _ = eng.forward(ps[:, :max(pl)].to(torch.int32).contiguous(), pl, False, stash=False)
            ids = ys[:, :L].to(torch.int32).contiguous()
            r = rows.to(torch.int64)
            r = (r // Lw) * L + r % Lw
            chunk = max(1, LM.MAX_TOKEN_ROWS // L)
            h = None
            for s0 in range(0, S, chunk):
                s1 = min(s0 + chunk, S)
                utt = torch.arange(s0, s1, device=ys.device) % B
                x, _ = eng.dec_forward(eouts.index_select(0, utt), elens_dev.index_select(0, utt), ids[s0:s1], yl[s0:s1], False, False,
                                       causal=False, head=False)
                g = x.index_select(0, (r - s0 * L).clamp_(0, (s1 - s0) * L - 1))
                h = g if h is None else torch.where(((r >= s0 * L) & (r < s1 * L)).unsqueeze(1), g, h)
            with eng._scope():
                A = eng.arena
                y, _, _ = ops.layernorm_fwd(h, A.p("decoder.norm.weight"), A.p("decoder.norm.bias"), 1e-12, False)
                return eng.head_logits(y.view(1, n, -1), "decoder.output")[0]

    def decode(self, ps, plens=None):
        """greedy hypotheses of the CTC head over the phone encoder (lm_type "pctc")"""
        if self.decoder_type != "ctc":
            raise NotImplementedError("emoasr_amd: P2W.decode needs the CTC decoder (lm_type='pctc')")
        ps, plens = self._trim(ps, plens)
        with torch.no_grad():
            eouts, elens, _ = self.encoder(ps, plens)
            hyps, _, _, _ = self.decoder.decode(eouts, elens)
        return hyps
