"""Golden N-best lists of the LAS beam search on PREFIXES of the three las_tiny utterances, from the reference implementation.

Runs ONLY in the authoring container (the reference cannot travel); writes the data-only fixture tests/golden/las_beam_tiny.npz.
tests/test_las_beam_batch_cpu.py checks the fixture, tests/test_las_beam_batch_gpu.py holds the batched device search
(engine/las.py:las_beam_search_batch) to it.

    python tests/golden/make_golden_las_beam.py

The decoder state and the encoder outputs are those of las_tiny ("sd/decoder.*", "decode/{b}/eouts"): nothing but results is
stored.  A case is (utterance u, its first n frames, beam width W, len_weight lw) under the key
"case/u{u}_t{n}/bw{W}_lw{lw}/{hyps, lens, scores, margin}"; "sets" (JSON) lists the searches and widths of the sets A, B and C
that the GPU test decodes as one batch each.  Every recorded case has a decision margin (make_golden_las.py:shadow_decode)
above 1e-3 -- the sets were chosen by measuring it; wider beams on the full utterances go down to 1e-5.
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
from make_golden_las import DEC, no_dropout, shadow_decode  # noqa: E402
from asr.modeling.decoders.las import LASDecoder  # noqa: E402

MARGIN = 1e-3
LEN_WEIGHTS = (0.0, 0.1)
# set -> (searches (utterance, frames), widths)
SETS = {"A": dict(searches=[(0, 50), (1, 41), (2, 32), (0, 33), (1, 1)], widths=[1, 2, 3, 4, 8, 10]),
        "B": dict(searches=[(0, 1), (1, 1), (2, 1), (0, 33)], widths=[16]),
        "C": dict(searches=[(0, 1), (1, 1)], widths=[32])}


def case_key(u, n, bw, lw):
    return f"case/u{u}_t{n}/bw{bw}_lw{lw}"


def main():
    las = load_npz("las_tiny")
    assert json.loads(bytes(las["config"]).decode()) == json.loads(json.dumps(DEC))
    dec = LASDecoder(make_params(DEC), phase="test")
    dec.load_state_dict({k[len("sd/decoder."):]: torch.from_numpy(las[k]) for k in las if k.startswith("sd/decoder.")})
    no_dropout(dec)
    dec.eval()
    utts = [torch.from_numpy(las[f"decode/{b}/eouts"])[None] for b in range(3)]
    assert [u.shape[1] for u in utts] == [50, 41, 32], [u.shape for u in utts]   # set A's first three searches are the uncut utterances
    out = {"sets": np.frombuffer(json.dumps(SETS, sort_keys=True).encode(), dtype=np.uint8)}
    worst = {}
    with torch.no_grad():
        for name, spec in SETS.items():
            for u, n in spec["searches"]:
                eo = utts[u][:, :n].contiguous()
                for bw in spec["widths"]:
                    for lw in LEN_WEIGHTS:
                        key = case_key(u, n, bw, lw)
                        if key + "/lens" in out:
                            continue
                        hyps, scores, _, _ = dec.decode(eo, torch.tensor([n]), beam_width=bw, len_weight=lw)
                        assert len(hyps) > 0, key
                        h2, s2, gap = shadow_decode(dec, eo, bw, lw)
                        assert h2 == hyps and np.allclose(s2, scores), key
                        assert gap > MARGIN, f"{key}: decision margin {gap:.2e}"
                        out[key + "/lens"] = np.array([len(h) for h in hyps])
                        out[key + "/hyps"] = np.array(sum(hyps, []), dtype=np.int64)
                        out[key + "/scores"] = np.array(scores, dtype=np.float64)
                        out[key + "/margin"] = np.array(gap)
                        worst[(name, bw)] = min(worst.get((name, bw), float("inf")), gap)
    for (name, bw), gap in sorted(worst.items()):
        print(f"set {name} W={bw}: smallest margin {gap:.3e}")
    save_npz("las_beam_tiny", out)


if __name__ == "__main__":
    main()
