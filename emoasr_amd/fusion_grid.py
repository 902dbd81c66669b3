"""Shallow-fusion grid search for CTC and attention models in ONE pass over the data (asr/fusion/test_fusion_grid.py).

The reference decodes the test set once per (lm_weight, len_weight) cell, 11 x 6 = 66 full decodes in 66 host processes.  Encoder,
head, soft-max and top-k do not depend on the cell, and the searches of all cells of a batch are independent: here every batch is
encoded once and all cells are searched in one call of ctc_prefix_beam_search_batch_lm (csrc/ctc_beam_lm.hip), each cell scored with
metrics.compute_wers on the device.  With a Transformer LM the tool sets decoder.ctc_tlm_fusion = "device" (set_ctc_tlm_fusion): the LM is
stepped over a prefix tree on the device (where that form cannot take the LM the reason is logged and the
per-frame lm.predict runs).

    results, best = ctc_fusion_grid(model, dataloader, vocab, beam_width, lm, lm_weights, len_weights, device)
    python -m emoasr_amd.fusion_grid -conf asr.yaml -ep 40 --data test.tsv --beam_width 10 --lm_conf lm.yaml --lm_ep 20

results = [(lm_weight, len_weight, wer, wer_info), ...], lm_weight outer and len_weight inner as the reference builds its cells;
best = the first cell whose WER is strictly below every earlier one's, starting from 100 (test_fusion_grid.py:51-64).

Attention models (decoder_type == "transformer", any --decode_ctc_weight) go through joint_fusion_grid: one encoder pass and one
joint_beam_search_device_grid call per batch -- every distinct lm_weight is searched once, the len_weights are an expansion of the
finished hypotheses' scores; with an RNN LM the tool sets decoder.joint_rnnlm_impl = "device", so that the LM is
stepped inside that search (section 26).  Transducer models (decoder_type == "rnn_transducer") go through
rnnt_fusion_grid: the RNN LM is fused inside the batched device search, one search per distinct lm_weight (section 25); with a
Transformer LM the tool sets decoder.rnnt_tlm_fusion = "device" and the LM is stepped there over a prefix tree (section 30; where
that form cannot take the LM the reason is logged and the host form runs).  LAS models
(decoder_type == "las") go through las_fusion_grid: the reference's LAS search ignores the LM, the tool sets decoder.las_lm_fusion =
"fuse" and the RNN LM is stepped inside the batched LAS search, one search per distinct lm_weight over frames stored once per
utterance (section 28); with a Transformer LM it also sets decoder.las_tlm_fusion = "device" and the LM is stepped there over a prefix
tree (section 33; where that form cannot take the LM the reason is logged and the host form runs).  main dispatches "las" itself;
grid_of keeps refusing it.
"""
import argparse
import logging
import os

import numpy as np
import torch

from .decode import strip_eos
from .metrics import compute_wers, wer_summary

EPS = 1e-5           # test_fusion_grid.py:17
GRID_BATCH = 16      # utterances per decode call of the command-line tool


def weight_lists(lm_min, lm_max, lm_step, len_min, len_max, len_step):
    """the reference's candidates (test_fusion_grid.py:39-40), as doubles, unrounded"""
    return np.arange(lm_min, lm_max + EPS, lm_step), np.arange(len_min, len_max + EPS, len_step)


def require_ctc(model, decode_ctc_weight=0):
    kind = getattr(model, "decoder_type", None)
    if kind != "ctc":
        raise NotImplementedError(f"emoasr_amd.fusion_grid handles CTC models only (decoder_type == 'ctc'), not {kind!r}")
    if decode_ctc_weight > 0:
        raise NotImplementedError("emoasr_amd.fusion_grid: decode_ctc_weight > 0 is the joint CTC / attention search, whose grid is "
                                  "not built; CTC models only")


def _grid_pass(model, dataloader, vocab, cells, search_batch, device, eos_id, decode_ctc_weight, texts_out, greedy_at_one):
    """one pass over the loader -> (results, best): every batch is encoded once, search_batch(eouts, elens) -> hyps[b][c] searches
    all cells of it (greedy_at_one and decode_ctc_weight == 1: greedy CTC whatever the weights, decoded once per batch for every
    cell), every cell is scored with compute_wers; best = the first cell with strictly smaller WER, from (0, 0, 100, "")"""
    hyps_of = [[] for _ in cells]
    refs = []
    with torch.no_grad():
        for data in dataloader:
            eouts, elens, eouts_inter = model.encoder(data["xs"].to(device), data["xlens"])
            if greedy_at_one and decode_ctc_weight == 1:
                greedy = model.decoder.decode(eouts, elens, eouts_inter, 1, decode_ctc_weight=1)[0]
                best_of = lambda b, c: greedy[b]
            else:
                hyps = search_batch(eouts, elens)
                best_of = lambda b, c: hyps[b][c][0] if hyps[b][c] else []
            for b, reftext in enumerate(data["texts"]):
                refs.append(reftext.split())
                for c in range(len(cells)):
                    hyps_of[c].append(vocab.ids2text(strip_eos(best_of(b, c), eos_id)).split())
    if texts_out is not None:
        texts_out += [[" ".join(words) for words in cell] for cell in hyps_of]
    results = []
    best = (0, 0, 100, "")
    for c, (lm_weight, len_weight) in enumerate(cells):
        wer, wer_dict = compute_wers(hyps_of[c], refs, device=device)
        row = (lm_weight, len_weight, wer, wer_summary(wer, wer_dict))
        results.append(row)
        if wer < best[2]:
            best = row
    return results, best


def _cells(lm_weights, len_weights):
    return [(np.float64(a), np.float64(b)) for a in lm_weights for b in len_weights]


def _require_kind(model, kind, name):
    got = getattr(model, "decoder_type", None)
    if got != kind:
        raise NotImplementedError(f"emoasr_amd.fusion_grid.{name} handles decoder_type == {kind!r}, not {got!r}")


def ctc_fusion_grid(model, dataloader, vocab, beam_width, lm, lm_weights, len_weights, device, eos_id=2, decode_ctc_weight=0,
                    texts_out=None):
    """-> (results, best): results = [(lm_weight, len_weight, wer, wer_info)] over lm_weights x len_weights (lm_weights outer), best =
    (lm_weight, len_weight, wer, wer_info) of the first cell with strictly smaller WER, from (0, 0, 100, "") as the reference starts.
    One pass over the loader: every batch is encoded once, all cells are searched in one call, a cell with lm_weight <= 0 is the search
    without an LM (it adds nothing).  texts_out: a list that receives, per cell in the order of results, the 1-best texts."""
    from .modeling.ctc_beam_search import ctc_prefix_beam_search_batch_lm
    require_ctc(model, decode_ctc_weight)
    cells = _cells(lm_weights, len_weights)
    search = lambda eouts, elens: ctc_prefix_beam_search_batch_lm(model.decoder, eouts, elens, beam_width, lm, cells)[0]
    return _grid_pass(model, dataloader, vocab, cells, search, device, eos_id, decode_ctc_weight, texts_out, False)


def joint_fusion_grid(model, dataloader, vocab, beam_width, lm, lm_weights, len_weights, device, eos_id=2, decode_ctc_weight=0,
                      texts_out=None):
    """ctc_fusion_grid for an attention model (decoder_type == "transformer"): -> (results, best) with the same cell order and the
    same rule for best.  One encoder pass and one joint_beam_search_device_grid call per batch; decode_ctc_weight == 1 is greedy
    CTC whatever the weights: decoded once per batch, every cell gets that result."""
    from .modeling.beam_search_device import joint_beam_search_device_grid
    _require_kind(model, "transformer", "joint_fusion_grid")
    search = lambda eouts, elens: joint_beam_search_device_grid(model.decoder, eouts, elens, beam_width, lm, [a for a in lm_weights],
                                                                [b for b in len_weights], decode_ctc_weight)[0]
    return _grid_pass(model, dataloader, vocab, _cells(lm_weights, len_weights), search, device, eos_id, decode_ctc_weight, texts_out,
                      True)


def rnnt_fusion_grid(model, dataloader, vocab, beam_width, lm, lm_weights, len_weights, device, eos_id=2, decode_ctc_weight=0,
                     texts_out=None):
    """joint_fusion_grid for a transducer model (decoder_type == "rnn_transducer"): -> (results, best) with the same cell order and
    the same rule for best.  One encoder pass and one engine.rnnt_beam_search_batch grid call per batch: every distinct positive
    lm_weight of an utterance is one search with the RNN LM stepped beside the prediction network, the len_weights are a host
    expansion.  decode_ctc_weight == 1 is greedy CTC whatever the weights, as in joint_fusion_grid."""
    from .modeling.functions import rnnt_fusion_grid_apply
    _require_kind(model, "rnn_transducer", "rnnt_fusion_grid")
    # decoder.rnnt_tlm_fusion = "device" (set_rnnt_tlm_fusion): a Transformer LM is stepped on the device over a prefix tree
    # (DESIGN.md section 30); "host", the default, is the call as it always was
    kw = {"tlm_fusion": "device"} if getattr(model.decoder, "rnnt_tlm_fusion", "host") == "device" else {}
    search = lambda eouts, elens: rnnt_fusion_grid_apply(model.decoder, eouts, elens, beam_width, lm, lm_weights, len_weights, **kw)[0]
    return _grid_pass(model, dataloader, vocab, _cells(lm_weights, len_weights), search, device, eos_id, decode_ctc_weight, texts_out,
                      True)


def las_fusion_grid(model, dataloader, vocab, beam_width, lm, lm_weights, len_weights, device, eos_id=2, decode_ctc_weight=0,
                    texts_out=None):
    """rnnt_fusion_grid for a LAS model (decoder_type == "las"): -> (results, best) with the same cell order and the same rule for
    best.  One encoder pass and one functions.las_fusion_grid_apply call per batch: every distinct positive lm_weight of an
    utterance is one search with the RNN LM stepped inside the chain, the searches of an utterance share its frames, the
    len_weights are a host expansion.  decode_ctc_weight == 1 is greedy CTC whatever the weights."""
    from .modeling.functions import las_fusion_grid_apply
    _require_kind(model, "las", "las_fusion_grid")
    search = lambda eouts, elens: las_fusion_grid_apply(model.decoder, eouts, elens, beam_width, lm, lm_weights, len_weights)[0]
    return _grid_pass(model, dataloader, vocab, _cells(lm_weights, len_weights), search, device, eos_id, decode_ctc_weight, texts_out,
                      True)


def grid_of(kind):
    """the grid function of a decoder type: "ctc" -> ctc_fusion_grid, "transformer" -> joint_fusion_grid, "rnn_transducer" ->
    rnnt_fusion_grid.  "las" stays refused here: main sends it to las_fusion_grid before it asks (the reference's LAS search
    ignores the LM; the fused one is this project's)"""
    if kind == "ctc":
        return ctc_fusion_grid
    if kind == "transformer":
        return joint_fusion_grid
    if kind == "rnn_transducer":
        return rnnt_fusion_grid
    raise NotImplementedError(f"emoasr_amd.fusion_grid handles decoder_type 'ctc' and 'transformer' (and 'rnn_transducer'), "
                              f"not {kind!r}")


def grid_for(kind):
    """main's dispatch: "las" -> las_fusion_grid, decided before grid_of is asked (which refuses it); every other type: grid_of"""
    return las_fusion_grid if kind == "las" else grid_of(kind)


def set_joint_rnnlm_impl(decoder, beam_width, lm, decode_ctc_weight):
    """an attention model with a stateful LM (the RNN LM): decoder.joint_rnnlm_impl = "device", every distinct lm_weight searched in one
    pass with the LM stepped on the device -- unless beam_search_device.batch_rnnlm_why_not gives a reason: that
    reason is logged and the switch stays "host" (one host search per utterance and weight).  -> the value set"""
    from .modeling.beam_search_device import batch_rnnlm_why_not
    impl = "host"
    if getattr(lm, "stateful", False):
        why = batch_rnnlm_why_not(decoder, beam_width, lm, decode_ctc_weight)
        if why is None:
            impl = "device"
        else:
            logging.info(f"joint_rnnlm_impl stays 'host' (one host search per utterance and lm_weight): {why}")
    decoder.joint_rnnlm_impl = impl
    return impl


def set_rnnt_tlm_fusion(decoder, beam_width, lm):
    """a transducer model with a Transformer LM: decoder.rnnt_tlm_fusion = "device", every distinct lm_weight of an utterance is one
    search with the LM stepped on the device over a prefix tree -- unless engine.rnnt_beam_tlm_why_not or the
    device search's limits give a reason: that reason is logged and the switch stays "host" (one host search per utterance and
    weight).  -> the value set"""
    from .modeling.functions import _engine_of
    impl = "host"
    if getattr(lm, "lm_type", None) == "transformer":
        eng = _engine_of(decoder)
        why = eng.rnnt_beam_tlm_why_not(lm)
        if why is None and not eng.rnnt_beam_device_ok(beam_width):
            why = f"the model or beam_width {beam_width} is outside the batched device search's limits"
        if why is None:
            impl = "device"
        else:
            logging.info(f"rnnt_tlm_fusion stays 'host' (one host search per utterance and lm_weight): {why}")
    decoder.rnnt_tlm_fusion = impl
    return impl


def set_ctc_tlm_fusion(decoder, lm):
    """a CTC model with a Transformer LM: decoder.ctc_tlm_fusion = "device", the LM is stepped on the device over a prefix tree
     -- unless functions.ctc_tlm_why_not gives a reason: that reason is logged and the switch stays "host"
    (one lm.predict over the new prefixes per frame).  -> the value set"""
    from .modeling.functions import ctc_tlm_why_not
    impl = "host"
    if getattr(lm, "lm_type", None) == "transformer":
        why = ctc_tlm_why_not(decoder, lm)
        if why is None:
            impl = "device"
        else:
            logging.info(f"ctc_tlm_fusion stays 'host' (one lm.predict over the new prefixes per frame): {why}")
    decoder.ctc_tlm_fusion = impl
    return impl


def set_las_lm_fusion(decoder, beam_width, lm):
    """a LAS model: decoder.las_lm_fusion = "fuse"; where functions.las_rnnlm_why_not gives a reason the grid runs one host search
    per utterance and lm_weight, and that reason is logged.  -> the reason or None"""
    from .modeling.functions import las_rnnlm_why_not, las_tlm_why_not
    decoder.las_lm_fusion = "fuse"
    if getattr(lm, "lm_type", None) == "transformer":
        # a Transformer LM: decoder.las_tlm_fusion = "device", the LM is stepped inside the batched search over the prefix tree
        #  -- unless las_tlm_why_not gives a reason: it is logged and the switch stays "host"
        why = las_tlm_why_not(decoder, beam_width, lm)
        decoder.las_tlm_fusion = "device" if why is None else "host"
        if why is None:
            return None
        logging.info(f"las_tlm_fusion stays 'host': {why}")
    why = las_rnnlm_why_not(decoder, beam_width, lm)
    if why is not None:
        logging.info(f"LAS fusion grid: the host form per utterance and lm_weight: {why}")
    return why


def log_results(results, best):
    """the reference's log lines (test_fusion_grid.py:56-69)"""
    for lm_weight, len_weight, _, wer_info in results:
        logging.info(f"lm_weight: {lm_weight:.3f} len_weight: {len_weight:.3f} - {wer_info}")
    logging.info("***** best WER:")
    logging.info(f"lm_weight: {best[0]:.3f} len_weight: {best[1]:.3f} - {best[3]}")


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m emoasr_amd.fusion_grid", description=__doc__.split("\n\n")[0])
    parser.add_argument("-conf", type=str, required=True)
    parser.add_argument("-ep", type=str, required=True)
    parser.add_argument("--data", type=str, default=None)
    parser.add_argument("--data_tag", type=str, default="test")
    parser.add_argument("--save_dir", type=str, default=None)
    parser.add_argument("--beam_width", type=int, default=None)
    parser.add_argument("--decode_ctc_weight", type=float, default=0)
    parser.add_argument("--lm_min", type=float, default=0)
    parser.add_argument("--lm_max", type=float, default=1)
    parser.add_argument("--lm_step", type=float, default=0.1)
    parser.add_argument("--len_min", type=float, default=0)
    parser.add_argument("--len_max", type=float, default=5)
    parser.add_argument("--len_step", type=float, default=1)
    parser.add_argument("--lm_conf", type=str, default=None)
    parser.add_argument("--lm_ep", type=str, default=None)
    parser.add_argument("--lm_tag", type=str, default=None)
    return parser


def _loader(dataset, n):
    for i in range(0, len(dataset), n):
        yield dataset.collate_fn([dataset[j] for j in range(i, min(i + n, len(dataset)))])


def main(args):
    from .datasets import ASRDataset, Vocab
    from .modeling.asr import ASR
    from .modeling.lm import LM
    from .rescore import load_config, model_path
    params = load_config(args.conf)
    kind = getattr(params, "decoder_type", None)
    grid = grid_for(kind)
    if kind == "ctc":
        require_ctc(params, args.decode_ctc_weight)
    if not (args.lm_conf and args.lm_ep):
        raise SystemExit("emoasr_amd.fusion_grid: shallow fusion needs --lm_conf and --lm_ep")
    device = torch.device("cuda")
    log_dir = args.save_dir or os.path.splitext(args.conf)[0]
    os.makedirs(log_dir, exist_ok=True)
    data_path = args.data or params.test_path
    data_tag = args.data if args.data_tag == "test" and data_path != args.data and args.data else args.data_tag
    data_tag = os.path.splitext(os.path.basename(data_tag))[0]
    logging.basicConfig(filename=os.path.join(log_dir, f"test_fusion_grid_{data_tag}_ctc{args.decode_ctc_weight}_ep{args.ep}.log"),
                        format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s", level=logging.INFO)
    model = ASR(params, phase="test")
    model.load_state_dict(torch.load(model_path(args.conf, args.ep), map_location="cpu"))
    model.to(device).eval()
    if kind == "ctc":
        model.decoder.ctc_beam_impl = "device"
    lm_params = load_config(args.lm_conf)
    lm = LM(lm_params, phase="test")
    lm.load_state_dict(torch.load(model_path(args.lm_conf, args.lm_ep), map_location="cpu"))
    lm.to(device).eval()
    beam_width = args.beam_width or params.beam_width
    if kind == "ctc":
        set_ctc_tlm_fusion(model.decoder, lm)
    if kind == "transformer":
        set_joint_rnnlm_impl(model.decoder, beam_width, lm, args.decode_ctc_weight)
    if kind == "las":
        set_las_lm_fusion(model.decoder, beam_width, lm)
    if kind == "rnn_transducer":
        set_rnnt_tlm_fusion(model.decoder, beam_width, lm)
    dataset = ASRDataset(params, data_path, phase="test")
    lm_weights, len_weights = weight_lists(args.lm_min, args.lm_max, args.lm_step, args.len_min, args.len_max, args.len_step)
    results, best = grid(model, _loader(dataset, GRID_BATCH), Vocab(params.vocab_path), beam_width,
                         lm, lm_weights, len_weights, device, eos_id=params.eos_id, decode_ctc_weight=args.decode_ctc_weight)
    log_results(results, best)
    return results, best


if __name__ == "__main__":
    main(build_parser().parse_args())
