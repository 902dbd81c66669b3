"""Digest of the transducer's searches on the l4_tiny golden model, to compare two commits on one machine: every
search form's hypotheses, every score as a hex double, and for every HIP graph captured on the way the sequence of C ABI entry points
its body issued.  Two commits that search alike write byte-identical files.  It uses engine and LM methods only.

    python tools/rnnt_search_digest.py --out profiles/rnnt_search_digest.json

Forms, in f32 and bf16: the launch chain; the replayed round with the fused body and (a second model, built under
EMOASR_RNNT_BEAM_FUSED=0) with the unfused one; the device batch without an LM; the RNN-LM and Transformer-LM grids at lm_weights
[0, 0.3] x len_weights [0, 0.5]; lockstep greedy at K = 1, 4, 8; lm.predict of the Transformer LM through its captured forward.  The
beam and greedy forms run over the golden utterances, each encoded alone; the grids and lm.predict over the first 12 / 5 / 0 frames of
the first three (the Transformer LM of the fixture holds 64 positions), as tests/test_rnnt_fusion_gpu.py does."""
import argparse
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tests.rnnlm_util import RNNLM_CFG, rnnlm_golden, rnnlm_state  # noqa: E402
from tests.util import CONFIGS, LM_CFG, RNNT_BEAM_WIDTHS, load_ctc_beam_golden, load_golden  # noqa: E402

GRID_ELENS = (12, 5, 0)
LM_WEIGHTS, LEN_WEIGHTS = [0.0, 0.3], [0.0, 0.5]


class CallLog:
    """lib.call wrapped for the tool's run: the entry names issued while the current stream is capturing, one list per capture"""

    def __init__(self):
        from emoasr_amd import lib
        self.lib, self.inner, self.captures, self.was_capturing = lib, lib.call, [], False
        lib.call = self

    def __call__(self, name, *args):
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and not self.was_capturing:
            self.captures.append([])
        self.was_capturing = capturing
        if capturing:
            self.captures[-1].append(name)
        return self.inner(name, *args)

    def take(self):
        """the captures since the last take"""
        out, self.captures, self.was_capturing = self.captures, [], False
        return out

    def close(self):
        self.lib.call = self.inner


def hexes(scores):
    return [hexes(s) if isinstance(s, (list, tuple)) else float(s).hex() for s in scores]


def build(dtype, dev):
    from emoasr_amd.modeling.asr import ASR
    _, sd, g = load_golden("l4_tiny")
    model = ASR(SimpleNamespace(**CONFIGS["l4_tiny"]), compute_dtype=dtype)
    model.load_state_dict(sd)
    return model.to(dev).eval(), g


def encode_alone(model, g, dev):
    outs = []
    for b in range(g["xs"].shape[0]):
        n = int(g["xlens"][b])
        eouts, elens, _ = model.encoder(g["xs"][b:b + 1, :n].to(dev), g["xlens"][b:b + 1])
        outs.append(eouts[0, :int(elens[0])])
    elens = [int(e.shape[0]) for e in outs]
    eouts = torch.zeros(len(outs), max(elens), outs[0].shape[1], device=dev, dtype=outs[0].dtype)
    for b, e in enumerate(outs):
        eouts[b, :elens[b]] = e
    return eouts, elens


def digest(dtype, dev, log):
    from emoasr_amd.modeling.lm import LM
    out = {}

    def record(name, hyps, scores=None, **more):
        out[name] = dict(hyps=hyps, captures=log.take(), **more)
        if scores is not None:
            out[name]["scores"] = hexes(scores)

    model, g = build(dtype, dev)
    eng, dec = model.engine(), model.decoder
    blank, eos = dec.blank_id, dec.eos_id
    eouts, elens = encode_alone(model, g, dev)
    utts = [eouts[b:b + 1, :n] for b, n in enumerate(elens)]
    for W in RNNT_BEAM_WIDTHS:
        for form in ("chain", "graph"):
            res = [getattr(eng, "_rnnt_beam_search_" + form)(e, W, blank, eos, return_scores=True) for e in utts]
            record(f"{form}-W{W}", [h for h, _ in res], [s for _, s in res])
        record(f"device-W{W}", *eng.rnnt_beam_search_batch(eouts, elens, W, blank, eos))
    for K in (1, 4, 8):
        hyps, aligns = eng.rnnt_greedy_batch(eouts, elens, blank, eos, frames_per_step=K)
        record(f"greedy-K{K}", hyps, aligns=aligns)

    os.environ["EMOASR_RNNT_BEAM_FUSED"] = "0"      # read when an engine builds its round record: a second model
    try:
        eng0 = build(dtype, dev)[0].engine()
        for W in RNNT_BEAM_WIDTHS:
            res = [eng0._rnnt_beam_search_graph(e, W, blank, eos, return_scores=True) for e in utts]
            record(f"graph-unfused-W{W}", [h for h, _ in res], [s for _, s in res], zero_copy=bool(eng0._beam_static.zero_copy))
    finally:
        del os.environ["EMOASR_RNNT_BEAM_FUSED"]

    rlm = LM(SimpleNamespace(**RNNLM_CFG), compute_dtype=dtype)
    rlm.load_state_dict(rnnlm_state(rnnlm_golden()))
    tlm = LM(SimpleNamespace(**LM_CFG), compute_dtype=dtype)
    tlm.load_state_dict(load_ctc_beam_golden()[2])
    rlm, tlm = rlm.to(dev).eval(), tlm.to(dev).eval()
    e3 = torch.stack([eouts[b, :GRID_ELENS[0]] for b in range(3)])
    for name, lm, how in (("rnnlm", rlm, "host"), ("tlm", tlm, "device")):
        for W in RNNT_BEAM_WIDTHS:
            record(f"grid-{name}-W{W}", *eng.rnnt_beam_search_batch(e3, list(GRID_ELENS), W, blank, eos, lm=lm, lm_weights=LM_WEIGHTS,
                                                                    len_weights=LEN_WEIGHTS, tlm_fusion=how))
    ys = torch.tensor([[eos, 5, 7, 9, 0, 0], [eos, 3, 0, 0, 0, 0], [eos, 11, 4, 6, 8, 10]])
    logp, _ = tlm.predict(ys, [4, 2, 6])
    record("lm-predict", [], logp.double().cpu().tolist())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    log = CallLog()
    try:
        with torch.no_grad():
            result = {name: digest(dtype, dev, log) for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16))}
    finally:
        log.close()
    # one line per (dtype, form), keys sorted: the file stays diffable line by line
    rows = sorted((f"{dt}/{name}", entry) for dt, forms in result.items() for name, entry in forms.items())
    text = "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True, separators=(',', ':'))}" for k, v in rows) + "\n}\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(json.dumps(dict(out=args.out, sha256=hashlib.sha256(text.encode()).hexdigest(), entries=sum(len(v) for v in result.values()))))


if __name__ == "__main__":
    main()
