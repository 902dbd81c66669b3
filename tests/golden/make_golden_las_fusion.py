"""Golden N-best lists of the LAS beam search WITH RNN-LM shallow fusion, from the reference's own modules.

Runs ONLY in the authoring container (the reference cannot travel); writes the data-only fixture tests/golden/las_fusion_tiny.npz.
tests/test_las_fusion_cpu.py checks the fixture, tests/test_las_fusion_gpu.py holds the fused searches to it.

    python tests/golden/make_golden_las_fusion.py

The reference's LAS search takes `lm` / `lm_weight` and never reads them (las.py:233 is `pass`); the fusion recorded here is the
one its attention search performs at decode_ctc_weight == 0 (decoders/transformer.py:217-226, 246-286), whose loop the end of the
LAS step repeats line for line: per live hypothesis  log_softmax(head) + lm_weight * lm.predict(last token, the hypothesis's own
LM state)[:, :V],  the top beam_width of that row, the sum as the score increment.  The loop below walks the reference's
LASDecoder.forward_one_step / output (decoder state of las_tiny) and the reference's RNNLM.predict (state of rnnlm_tiny; both
V = 40) and measures the decision margin as make_golden_las.py:shadow_decode does.

The searches are set A of las_beam_tiny.  A case is "case/u{u}_t{n}/bw{W}_lw{lw}_lm{a}/{hyps, lens, scores, margin}"; "groups" (JSON)
lists the recorded (lm_weight, widths).  Every recorded case has a margin above 1e-3, and in every (W, lm_weight) group the fused
N-best list differs from las_beam_tiny's unfused one in at least one search: both are asserted here.  Groups that fall under the
bar on some search -- lm_weight 0.3 at W 4 / 8, 1.0 at W >= 3, 0.1 at W 1 / 4 / 8 / 10 -- are left out, not skipped at test time.
"""
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_npz, make_params, save_npz  # noqa: E402  (puts the reference on sys.path)
from make_golden_las import DEC, no_dropout  # noqa: E402
from make_golden_las_beam import SETS, case_key  # noqa: E402
from asr.modeling.decoders.las import LASDecoder  # noqa: E402
from utils.converters import strip_eos  # noqa: E402
from lm.modeling.lm import LM  # noqa: E402

sys.path.insert(1, os.path.dirname(os.path.dirname(HERE)))
from tests.rnnlm_util import RNNLM_CFG  # noqa: E402

MARGIN = 1e-3
LEN_WEIGHTS = (0.0, 0.1)
SEARCHES = SETS["A"]["searches"]
GROUPS = [(0.5, [1, 3, 4, 8, 10]), (0.3, [1, 3, 10]), (0.1, [3]), (1.0, [1])]      # (lm_weight, widths)


def fusion_key(u, n, bw, lw, a):
    return f"{case_key(u, n, bw, lw)}_lm{a}"


def fused_decode(dec, lm, eouts, beam_width, len_weight, lm_weight):
    """shadow_decode (make_golden_las.py) with the attention search's LM term -> (hyps, scores, gap)"""
    gap = float("inf")
    V = DEC["vocab_size"]
    beams = [dict(hyp=[dec.eos_id], score=0.0, ctx=eouts.new_zeros(1, 1, dec.enc_hidden_size), dstate=None, aw=None, lm_states=None)]
    results = []
    for i in range(dec.max_decode_ylen):
        new_beams, spare = [], []
        for beam in beams:
            y_emb = dec.dropout_emb(dec.embed(torch.tensor([[beam["hyp"][-1]]])))
            logit, ctx, dstate, aw = dec.forward_one_step(y_emb, beam["ctx"], eouts, beam["dstate"], beam["aw"])
            scores = torch.log_softmax(dec.output(logit).squeeze(0), dim=-1)
            scores_lm, lm_states = lm.predict(torch.tensor([beam["hyp"]]), torch.tensor([i + 1]), states=beam["lm_states"])
            scores = scores + lm_weight * scores_lm[:, :V]
            top, idx = torch.topk(scores, k=beam_width + 1, dim=1)
            spare.append(beam["score"] + float(top[0, beam_width]))
            for j in range(beam_width):
                new_beams.append(dict(hyp=beam["hyp"] + [int(idx[0, j])], score=beam["score"] + float(top[0, j]), ctx=ctx,
                                      dstate=dstate, aw=aw, lm_states=lm_states))
        ranked = sorted(new_beams, key=lambda x: x["score"], reverse=True)
        gap = min(gap, ranked[:beam_width][-1]["score"] - max([x["score"] for x in ranked[beam_width:]] + spare))
        beams, extend = ranked[:beam_width], []
        for beam in beams:
            if beam["hyp"][-1] == dec.eos_id:
                hyp = strip_eos(beam["hyp"], dec.eos_id)
                if len(hyp) < 1:
                    continue
                results.append(dict(hyp=hyp, score=beam["score"] + len_weight * len(beam["hyp"])))
                if len(results) >= beam_width:
                    break
            else:
                extend.append(beam)
        if len(results) >= beam_width or not extend:
            break
        beams = extend
    results = sorted(results, key=lambda x: x["score"], reverse=True)
    sc = [r["score"] for r in results]
    gap = min([gap] + [a - b for a, b in zip(sc[:-1], sc[1:])])
    return [r["hyp"] for r in results], sc, gap


def main():
    las, unfused, rl = load_npz("las_tiny"), load_npz("las_beam_tiny"), load_npz("rnnlm_tiny")
    dec = LASDecoder(make_params(DEC), phase="test")
    dec.load_state_dict({k[len("sd/decoder."):]: torch.from_numpy(las[k]) for k in las if k.startswith("sd/decoder.")})
    no_dropout(dec)
    dec.eval()
    lm = LM(make_params(RNNLM_CFG))
    lm.load_state_dict({k[3:]: torch.from_numpy(rl[k]) for k in rl if k.startswith("sd/")})
    lm.lm.rnns.dropout = 0.0
    lm.eval()
    assert RNNLM_CFG["vocab_size"] == DEC["vocab_size"] == 40
    utts = [torch.from_numpy(las[f"decode/{b}/eouts"])[None] for b in range(3)]
    out = {"groups": np.frombuffer(json.dumps(GROUPS).encode(), dtype=np.uint8),
           "searches": np.array(SEARCHES, dtype=np.int64), "len_weights": np.array(LEN_WEIGHTS)}
    with torch.no_grad():
        for a, widths in GROUPS:
            for bw in widths:
                worst, changed, best_changed = float("inf"), 0, 0
                for u, n in SEARCHES:
                    eo = utts[u][:, :n].contiguous()
                    for lw in LEN_WEIGHTS:
                        key = fusion_key(u, n, bw, lw, a)
                        hyps, scores, gap = fused_decode(dec, lm, eo, bw, lw, a)
                        assert len(hyps) > 0, key
                        assert gap > MARGIN, f"{key}: decision margin {gap:.2e}"
                        out[key + "/lens"] = np.array([len(h) for h in hyps])
                        out[key + "/hyps"] = np.array(sum(hyps, []), dtype=np.int64)
                        out[key + "/scores"] = np.array(scores, dtype=np.float64)
                        out[key + "/margin"] = np.array(gap)
                        worst = min(worst, gap)
                        base = case_key(u, n, bw, lw)
                        lens0 = unfused[base + "/lens"].tolist()
                        flat0 = unfused[base + "/hyps"].tolist()
                        if lw == 0.0:
                            changed += (lens0, flat0) != ([len(h) for h in hyps], sum(hyps, []))
                            best_changed += flat0[:lens0[0]] != hyps[0]
                assert changed >= 1, f"lm_weight {a} W {bw}: the LM changes no N-best list"
                print(f"lm_weight {a} W={bw}: smallest margin {worst:.3e}; N-best changed in {changed} of {len(SEARCHES)} searches, "
                      f"1-best in {best_changed}")
    save_npz("las_fusion_tiny", out)


if __name__ == "__main__":
    main()
