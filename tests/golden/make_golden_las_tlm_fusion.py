"""Golden N-best lists of the LAS beam search WITH Transformer-LM shallow fusion, from the reference's own
modules.

Runs ONLY in the authoring container (the reference cannot travel); writes the data-only fixture tests/golden/las_tlm_fusion_tiny.npz.
tests/test_las_tlm_fusion_cpu.py checks the fixture, tests/test_las_tlm_fusion_gpu.py holds the fused searches to it.

    python tests/golden/make_golden_las_tlm_fusion.py

The loop is make_golden_las_fusion.py's fused_decode -- the reference's LASDecoder.forward_one_step / output (decoder state of
las_tiny) with the LM term of the reference's attention search -- with the reference's Transformer LM in place of its RNN LM:
lm.predict on the hypothesis's whole prefix (LM_CFG, the `lm/` state of l3_tiny; both V = 40).  The searches are set A of
las_beam_tiny, the keys las_fusion_tiny's.  Every recorded case has a margin above 1e-3, and in every (W, lm_weight) group the fused
N-best list differs from las_beam_tiny's unfused one in at least one search: both are asserted here.  Pairs that fall under the bar on
some search -- 0.1 / 0.3 / 0.4 / 0.5 / 0.7 / 1.0 / 1.5 at W 8 or 10, 0.5 at W 4, 0.05 at W 8, 0.2 at W 10 -- are left out, not skipped
at test time.
"""
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import LM_CFG, load_npz, make_params, save_npz  # noqa: E402  (puts the reference on sys.path)
from make_golden_las import DEC, no_dropout  # noqa: E402
from make_golden_las_beam import SETS, case_key  # noqa: E402
from make_golden_las_fusion import fused_decode, fusion_key  # noqa: E402
from asr.modeling.decoders.las import LASDecoder  # noqa: E402
from lm.modeling.lm import LM  # noqa: E402

MARGIN = 1e-3
LEN_WEIGHTS = (0.0, 0.1)
SEARCHES = SETS["A"]["searches"]
GROUPS = [(0.1, [3, 4]), (0.3, [3, 4]), (0.5, [3]), (1.0, [1, 3, 4]), (0.2, [8]), (0.05, [10]), (2.0, [8, 10])]   # (lm_weight, widths)


def main():
    las, unfused, l3 = load_npz("las_tiny"), load_npz("las_beam_tiny"), load_npz("l3_tiny")
    dec = LASDecoder(make_params(DEC), phase="test")
    dec.load_state_dict({k[len("sd/decoder."):]: torch.from_numpy(las[k]) for k in las if k.startswith("sd/decoder.")})
    no_dropout(dec)
    dec.eval()
    lm = LM(make_params(LM_CFG))
    lm.load_state_dict({k[3:]: torch.from_numpy(l3[k]) for k in l3 if k.startswith("lm/")})
    lm.eval()
    assert LM_CFG["vocab_size"] == DEC["vocab_size"] == 40
    utts = [torch.from_numpy(las[f"decode/{b}/eouts"])[None] for b in range(3)]
    out = {"groups": np.frombuffer(json.dumps(GROUPS).encode(), dtype=np.uint8),
           "searches": np.array(SEARCHES, dtype=np.int64), "len_weights": np.array(LEN_WEIGHTS)}
    longest = 0
    with torch.no_grad():
        for a, widths in GROUPS:
            for bw in widths:
                worst, changed = float("inf"), 0
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
                        longest = max([longest] + [len(h) for h in hyps])
                        base = case_key(u, n, bw, lw)
                        if lw == 0.0:
                            changed += (unfused[base + "/lens"].tolist(), unfused[base + "/hyps"].tolist()) != \
                                ([len(h) for h in hyps], sum(hyps, []))
                assert changed >= 1, f"lm_weight {a} W {bw}: the LM changes no N-best list"
                print(f"lm_weight {a} W={bw}: smallest margin {worst:.3e}; N-best changed in {changed} of {len(SEARCHES)} searches")
    print(f"longest hypothesis: {longest} tokens")
    save_npz("las_tlm_fusion_tiny", out)


if __name__ == "__main__":
    main()
