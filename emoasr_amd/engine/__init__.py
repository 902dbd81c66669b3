"""Explicit forward/backward sequencing of the HIP kernels.  CTCEngine (encoder.py: front-end, Transformer / Conformer encoder, CTC
head) inherits from one class per further part -- transformer_decoder.py, rnnt.py (over rnnt_search.py, the transducer's searches),
rnn_encoder.py, las.py; arena.py holds what they share."""
from .arena import (ArenaView, AttnStash, ConvStash, FFNStash, LayerRecord, ParamArena, _Stash, _cfg, arena_of, h2d_i32,  # noqa: F401
                    h2d_pack, sinusoid)
from .encoder import ASREngine, CTCEngine  # noqa: F401
