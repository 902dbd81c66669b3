"""Golden vectors of the LAS decoder (decoder_type "las", asr/modeling/decoders/las.py) from the reference at /root/reference.

Runs ONLY in the authoring container (the reference cannot travel); writes the data-only fixture tests/golden/las_tiny*.npz through
save_golden_npz.  tests/test_las_cpu.py pins tests/las_ref.py (the project's float64 restatement) against it, and
tests/test_las_gpu.py pins the HIP engine against it.

    python tests/golden/make_golden_las.py

ONE decoder state is used throughout (keys "sd/decoder.*"): the reference LASDecoder fitted for a few hundred CPU Adam steps to
three utterances of the l3_tiny encoder, so that beam search has real decisions to make and ends its hypotheses.  Every
nn.Dropout runs with p = 0 (the attention's dropout has a hard-coded p = 0.1 that no config field reaches).
"""
import copy
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ASR, L3, load_npz, make_batch, make_params, save_npz  # noqa: E402  (puts the reference on sys.path)
from asr.modeling.decoders.las import LASDecoder  # noqa: E402
from utils.converters import strip_eos  # noqa: E402

DEC = dict(vocab_size=40, embedding_size=64, enc_hidden_size=128, dec_hidden_size=96, dec_num_layers=2, attn_dim=80,
           dec_intermediate_size=112, dropout_dec_rate=0.0, lsm_prob=0.1, loss_normalize_length=False, loss_normalize_batch=True,
           kd_weight=0, mtl_ctc_weight=0.3, eos_id=2, blank_id=0, max_decode_ylen=20, mtl_phone_ctc_weight=0,
           mtl_inter_ctc_weight=0)
BATCHES = {"a": dict(T=37, elens=[37, 1, 20, 33], ylens=[5, 1, 9, 3], seed=11),
           "b": dict(T=211, elens=[211, 150], ylens=[3, 2], seed=12)}
DECODE = [(1, 0.0), (1, 0.1), (4, 0.0), (4, 0.1)]
KD = dict(kd_weight=0.5, reduce_main_loss_kd=False, kd_ctc_soft_label_weight=1.0, kd_ctc_position="all")   # (the CTC head reads the last three)
MARGIN = 1e-3
FIT_SEED, FIT_STEPS = 0, 300


def no_dropout(m):
    for s in m.modules():
        if isinstance(s, torch.nn.Dropout):
            s.p = 0.0


def decoder_batch(spec, V, D):
    g = torch.Generator().manual_seed(spec["seed"])
    elens, ylens = torch.tensor(spec["elens"]), torch.tensor(spec["ylens"])
    B, T, L = len(elens), spec["T"], int(ylens.max())
    eouts = torch.randn(B, T, D, generator=g)
    ys = torch.randint(3, V, (B, L), generator=g)
    for b in range(B):
        ys[b, ylens[b]:] = 2
    eos = torch.full((B, 1), 2)
    ys_in, ys_out = torch.cat([eos, ys], 1), torch.cat([ys, eos], 1)
    return eouts, elens, ys, ylens, ys_in, ys_out


def record(out, key, dec, batch, soft=None):
    """a float64 run of the reference decoder: losses (kept as float64), logits, every parameter gradient and eouts.grad (stored
    rounded to float32: 6e-8 relative, four orders below the tightest bar that reads them)"""
    eouts, elens, ys, ylens, ys_in, ys_out = batch
    torch.set_default_dtype(torch.float64)   # (the reference creates the LSTM state with the default dtype, las.py:147-152)
    try:
        d64 = copy.deepcopy(dec).double().train()
        e64 = eouts.double().requires_grad_(True)
        loss, loss_dict, logits = d64(e64, elens, None, ys, ylens, ys_in, ys_out, None if soft is None else soft.double())
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    out[f"{key}/eouts"], out[f"{key}/elens"] = eouts.numpy(), elens.numpy()
    out[f"{key}/ys"], out[f"{key}/ylens"] = ys.numpy(), ylens.numpy()
    out[f"{key}/ys_in"], out[f"{key}/ys_out"] = ys_in.numpy(), ys_out.numpy()
    if soft is not None:
        out[f"{key}/soft"] = soft.numpy()
    for k, v in loss_dict.items():
        out[f"{key}/{k}"] = torch.as_tensor(v).detach().numpy()
    out[f"{key}/logits"] = logits.detach().float().numpy()
    out[f"{key}/deouts"] = e64.grad.float().numpy()
    for n, p in d64.named_parameters():
        out[f"{key}/grad/decoder.{n}"] = p.grad.float().numpy()
    print(key, {k: float(v) for k, v in loss_dict.items()}, "w_score.bias.grad", float(d64.score.w_score.bias.grad.abs().max()))


def shadow_decode(dec, eouts, beam_width, len_weight):
    """the reference's search (las.py:176-287) walked once more through the reference's own forward_one_step, to MEASURE the
    smallest score gap at any decision: at every step between the last kept expansion and the best one that is not kept (the
    first dropped one of the sort, or a beam's (beam_width + 1)-th token, which a perturbed run could offer instead), and between
    the final results -> (hyps, scores, gap)"""
    gap = float("inf")

    def adjacent(vals):
        return min([a - b for a, b in zip(vals[:-1], vals[1:])], default=float("inf"))

    beams = [dict(hyp=[dec.eos_id], score=0.0, ctx=eouts.new_zeros(1, 1, dec.enc_hidden_size), dstate=None, aw=None)]
    results = []
    for _ in range(dec.max_decode_ylen):
        new_beams, spare = [], []
        for beam in beams:
            y_emb = dec.dropout_emb(dec.embed(torch.tensor([[beam["hyp"][-1]]])))
            logit, ctx, dstate, aw = dec.forward_one_step(y_emb, beam["ctx"], eouts, beam["dstate"], beam["aw"])
            scores = torch.log_softmax(dec.output(logit).squeeze(0), dim=-1)
            top, idx = torch.topk(scores, k=beam_width + 1, dim=1)
            spare.append(beam["score"] + float(top[0, beam_width]))
            for j in range(beam_width):
                new_beams.append(dict(hyp=beam["hyp"] + [int(idx[0, j])], score=beam["score"] + float(top[0, j]), ctx=ctx,
                                      dstate=dstate, aw=aw))
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
        if len(results) >= beam_width:
            break
        beams = extend
    results = sorted(results, key=lambda x: x["score"], reverse=True)
    gap = min(gap, adjacent([r["score"] for r in results]))
    return [r["hyp"] for r in results], [r["score"] for r in results], gap


def main():
    out = {"config": np.frombuffer(json.dumps(DEC, sort_keys=True).encode(), dtype=np.uint8)}
    l3 = load_npz("l3_tiny")
    model = ASR(make_params(L3), phase="train")
    model.load_state_dict({k[3:]: torch.from_numpy(l3[k]) for k in l3 if k.startswith("sd/")})
    xs, xlens, ys, ylens, ys_in, ys_out = make_batch(1, L3["feat_dim"], L3["vocab_size"])

    # a random-init decoder ends its hypotheses wherever chance has it: fit it, so that the search has real decisions to make
    torch.manual_seed(FIT_SEED)
    dec = LASDecoder(make_params(DEC), phase="train")
    no_dropout(dec)
    model.eval()
    utts = []
    with torch.no_grad():
        for b in range(3):
            eo, el, _ = model.encoder(xs[b:b + 1, : xlens[b]], xlens[b:b + 1])
            utts.append((eo, el))

    dec.train()
    opt = torch.optim.Adam(dec.parameters(), lr=2e-3)
    for step in range(FIT_STEPS):
        opt.zero_grad()
        total = 0.0
        for b, (eo, el) in enumerate(utts):
            n = int(ylens[b])
            loss, _, _ = dec(eo, el, None, ys[b:b + 1, :n], ylens[b:b + 1], ys_in[b:b + 1, : n + 1], ys_out[b:b + 1, : n + 1])
            total = total + loss
        total.backward()
        opt.step()
    print("fit: loss", float(total))
    for k, v in dec.state_dict().items():
        out["sd/decoder." + k] = v.detach().clone().numpy()

    # ---- decoding: beam 1 and 4, len_weight 0 and 0.1, on the three fitted utterances
    dec.eval()
    with torch.no_grad():
        for b, (eo, el) in enumerate(utts):
            out[f"decode/{b}/eouts"] = eo[0].numpy()
            for bw, lw in DECODE:
                hyps, scores, _, _ = dec.decode(eo, el, beam_width=bw, len_weight=lw)
                assert len(hyps) > 0, (b, bw, lw)
                h2, s2, gap = shadow_decode(dec, eo, bw, lw)
                assert h2 == hyps and np.allclose(s2, scores), (b, bw, lw)
                assert gap > MARGIN, f"utterance {b}, beam {bw}, len_weight {lw}: decision margin {gap:.2e} (change FIT_SEED)"
                key = f"decode/{b}/bw{bw}_lw{lw}"
                out[key + "/lens"] = np.array([len(h) for h in hyps])
                out[key + "/hyps"] = np.array(sum(hyps, []), dtype=np.int64)
                out[key + "/scores"] = np.array(scores, dtype=np.float64)
                out[key + "/margin"] = np.array(gap)
                print(key, hyps[0], f"margin {gap:.3e}")

    # ---- teacher-forced goldens in float64
    dec.train()
    for name, spec in BATCHES.items():
        record(out, name, dec, decoder_batch(spec, DEC["vocab_size"], DEC["enc_hidden_size"]))
    kd = LASDecoder(make_params(dict(DEC, **KD)), phase="train")
    no_dropout(kd)
    kd.load_state_dict(dec.state_dict())
    kd.train()
    batch = decoder_batch(BATCHES["a"], DEC["vocab_size"], DEC["enc_hidden_size"])
    g = torch.Generator().manual_seed(21)
    soft = torch.softmax(2.0 * torch.randn(batch[4].shape[0], batch[4].shape[1], DEC["vocab_size"], generator=g), dim=-1)
    record(out, "kd", kd, batch, soft)

    # ---- end to end: the l3_tiny encoder (weights in that fixture) under this decoder, float32 like the other model goldens
    model.decoder = dec
    model.train()
    model.zero_grad()
    loss, loss_dict = model(xs, xlens, ys, ylens, ys_in, ys_out)
    loss.backward()
    for k, v in loss_dict.items():
        out[f"e2e/{k}"] = torch.as_tensor(v).detach().numpy()
    for n in ("encoder.conv.conv.0.weight", "encoder.transformers.0.self_attn.linear_q.weight", "encoder.transformers.1.norm_final.weight"):
        out[f"e2e/grad/{n}"] = dict(model.named_parameters())[n].grad.numpy()
    model.eval()
    with torch.no_grad():
        hyps, scores, _, _ = model.decode(xs[0:1, : xlens[0]], xlens[0:1], beam_width=4)
    assert len(hyps) > 0
    out["e2e/hyp"] = np.array(hyps[0], dtype=np.int64)
    out["e2e/score"] = np.array(scores[0])
    print("e2e", {k: float(v) for k, v in loss_dict.items()}, hyps[0])
    save_npz("las_tiny", out)


if __name__ == "__main__":
    main()
