"""Batched CTC error correction against correct_step looped over the same utterances.

    python tools/correct_bench.py [--calls 20] [--warmup 5] [--repeats 5] [--batches 1,16,64] [--grid-batch 16]

Prints one JSON line.  Sizes of tools/lm_bench.py's correct_step_timing: the 23 M Conformer-CTC of bench.py with a hierarchical phone
head, the pbert of DESIGN.md section 14, bf16, 1 203 input frames = T' = 300 per utterance; random weights, the word head sharpened
and the blank's bias bisected until the first utterance's greedy hypothesis has about 40 tokens.
  cell["B{B}"]     ms per utterance of ONE cell (mask_th 0.9, lm_weight 0.5): `batch` = correct_batch on the B utterances, `loop` =
                   correct_step once per utterance (the code of the commit before the batch path: the baseline);
  grid             a 5 x 5 grid on --grid-batch utterances: `batch` = one correct_batch, `loop` = 25 looped evaluations, ms per
                   utterance of the whole grid;
  logits_at        us of P2W.logits_at on the masked rows of one threshold against the all-rows forward on the same inputs, and the
                   masked share of the token rows.
Protocol: device events around --calls calls after --warmup warm-ups, --repeats repeats (median, min, max), one process.
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, PV, FRAMES, TOKENS = 10872, 45, 1203, 40
ASR_CFG = dict(input_layer="conv2d", feat_dim=80, num_framestacks=1, encoder_type="conformer", decoder_type="ctc",
               pos_encode_type="rel", enc_hidden_size=256, enc_num_attention_heads=4, enc_num_layers=12, enc_intermediate_size=1024,
               dropout_enc_rate=0.1, dropout_attn_rate=0.1, vocab_size=V, blank_id=0, eos_id=2, kd_weight=0,
               mtl_phone_ctc_weight=0.3, hie_mtl_phone=True, phone_vocab_size=PV, inter_ctc_layer_id=6)
LM_CFG = dict(lm_type="pbert", input_layer="embed", enc_hidden_size=256, enc_num_attention_heads=4, enc_num_layers=4,
              enc_intermediate_size=1024, dec_hidden_size=256, dec_num_attention_heads=4, dec_num_layers=4,
              dec_intermediate_size=1024, dropout_enc_rate=0.1, dropout_dec_rate=0.1, dropout_attn_rate=0.1, mtl_ctc_weight=0,
              lsm_prob=0, kd_weight=0, max_decode_ylen=256, vocab_size=V, src_vocab_size=PV, max_seq_len=256, eos_id=2,
              mask_id=V - 1, phone_eos_id=2, phone_mask_id=PV - 2, blank_id=0, add_sos_eos=False)
GRID = [0.5, 0.7, 0.8, 0.9, 0.95], [0.0, 0.25, 0.5, 0.75, 1.0]


def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--grid-batch", type=int, default=16)
    a = ap.parse_args()
    from emoasr_amd.correct import correct_batch, correct_step
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.p2w import P2W
    dev = torch.device("cuda")
    torch.manual_seed(2)
    asr = ASR(SimpleNamespace(**ASR_CFG), phase="test", compute_dtype=torch.bfloat16).to(dev).eval()
    lm = P2W(SimpleNamespace(**LM_CFG), phase="test", compute_dtype=torch.bfloat16).to(dev).eval()
    batches = [int(x) for x in a.batches.split(",")]
    n_utts = max(batches + [a.grid_batch])
    xs = torch.randn(n_utts, FRAMES, 80)
    xlens = torch.full((n_utts,), FRAMES)
    with torch.no_grad():
        asr.decoder.output.weight.mul_(20.0)
        asr.decoder.phone_output.weight.mul_(20.0)
        lo, hi = -2000.0, 2000.0
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            asr.decoder.output.bias[0] = mid
            n = len(asr.decode(xs[:1].to(dev), xlens[:1])[0][0])
            if n == TOKENS:
                break
            lo, hi = (mid, hi) if n > TOKENS else (lo, mid)

    def batch_of(B):
        return {"utt_ids": [f"utt-{b}" for b in range(B)], "xs": xs[:B], "xlens": xlens[:B], "texts": [""] * B}

    singles = [{"utt_ids": [f"utt-{b}"], "xs": xs[b:b + 1], "xlens": xlens[b:b + 1], "texts": [""]} for b in range(n_utts)]

    def timed(fn, per):
        """ms per `per` of one call: events around --calls calls, --repeats times"""
        for _ in range(a.warmup):
            fn()
        out = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / a.calls / per)
        return out

    res = {"frames": 300, "dtype": "bf16", "lm": "pbert", "calls": a.calls, "warmup": a.warmup, "repeats": a.repeats, "cell": {}}
    for B in batches:
        data, det = batch_of(B), {}
        cells = correct_batch(asr, lm, data, 0, V - 1, 0.9, 0.5, dev, V, details=det)
        tb = timed(lambda: correct_batch(asr, lm, data, 0, V - 1, 0.9, 0.5, dev, V), B)
        tl = timed(lambda: [correct_step(asr, lm, d, 0, V - 1, 0.9, 0.5, dev, V) for d in singles[:B]], B)
        res["cell"][f"B{B}"] = dict(tokens=sum(t[5] for t in cells[0][0]), masked=sum(t[4] for t in cells[0][0]),
                                    batch_ms_per_utt=stats(tb), loop_ms_per_utt=stats(tl),
                                    loop_over_batch=[round(y / x, 3) for x, y in zip(tb, tl)])

    B = a.grid_batch
    data, (ths, ws) = batch_of(B), GRID
    tb = timed(lambda: correct_batch(asr, lm, data, 0, V - 1, ths, ws, dev, V), B)
    tl = timed(lambda: [correct_step(asr, lm, d, 0, V - 1, th, w, dev, V) for th in ths for w in ws for d in singles[:B]], B)
    res["grid"] = dict(B=B, mask_ths=ths, lm_weights=ws, batch_ms_per_utt=stats(tb), loop_ms_per_utt=stats(tl),
                       loop_over_batch=[round(y / x, 3) for x, y in zip(tb, tl)])

    # ---- the LM head on the masked rows against the all-rows forward, on the inputs of one threshold
    det = {}
    correct_batch(asr, lm, data, 0, V - 1, 0.9, 0.5, dev, V, details=det)
    ntok = [max(int(v), 1) for v in det["ntok"].cpu()]
    plens = [max(len(p), 1) for p in det["hyp_phone"]]
    ys, rows = det["ys"][0], det["lm_rows"]
    ps = torch.zeros(B, max(plens), dtype=torch.int64)
    for b, p in enumerate(det["hyp_phone"]):
        ps[b, :len(p)] = torch.from_numpy(p)
    ps_dev, ys_host = ps.to(dev), ys[:, :max(ntok)].cpu().long()
    t_at = timed(lambda: lm.logits_at(ys, ntok, rows, ps_dev, plens), 1e-3)
    t_all = timed(lambda: lm(ys_host, ntok, ps=ps, plens=plens), 1e-3)
    res["logits_at"] = dict(B=B, token_rows=sum(ntok), masked_rows=int(rows.numel()), logits_at_us=stats(t_at), forward_us=stats(t_all),
                            forward_over_logits_at=[round(y / x, 3) for x, y in zip(t_at, t_all)])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
