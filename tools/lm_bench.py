"""Transformer-LM training throughput and the vocabulary head A/B (fused = no [rows, V] logits, against materialised).

    python tools/lm_bench.py [--steps 20] [--warmup 5] [--pairs 5] [--batch 100] [--leg transformer|bert|electra|pbert|pelectra]

Prints one JSON line.  --leg transformer (the default):
  train_tokens_per_s   real (unpadded) tokens per second of a full training step (forward, backward, clip + AdamW) of the 12-layer
                       LM of bench.py (LM12: V = 10 000, d = 256) in bf16 at `--batch` sequences with Libri-like lengths, with the
                       head the gates select, and the same with the materialised head (EMOASR_CE_HEAD_FUSED=0's path);
  head_*_us            the head alone (loss rows forward + dX / dW / dbias backward) on that batch's rows, as same-box A/B pairs in
                       ONE process: fused, materialised, fused, ... -- the medians and every pair's ratio.

--leg bert: the BERT masked LM (lm_type="bert") at the same size, bf16:
  score                LM.masked_logprobs of a `--batch`-hypothesis Libri-like list for three values of max_token_rows: masked
                       copies per second and token rows (copies x padded length) per second, host time from the call to the
                       synchronised result (the upload, every chunk and the one copy back included), median of --pairs runs;
  mlm_step             real tokens per second of a full masked-LM training step at mask_proportion 0.15 and 0.3 with transform +
                       vocabulary head on the labelled rows only (LM.head_at_labels) against the head on all rows with row weights,
                       as alternating legs in ONE process -- the medians and every pair's ratio.

--leg electra: ELECTRA (lm_type="electra") at the size of the reference's recipe (12 + 12 layers, d = 256, V = 9 798, batch 90,
num_to_mask 35, electra_disc_weight 50), bf16:
  step                 a full training step (train_lm.train_step: generator, sampling, corruption, discriminator, both backwards,
                       clip + AdamW) with the sampling kernels (LM.sample_path = "hip": sample_rows + electra_corrupt) against the
                       comparator (LM.sample_path = "torch": softmax + torch.multinomial + indexed assignment, all on the device),
                       as alternating legs of --steps steps after --warmup in ONE process, --pairs pairs: median, min, max and every
                       pair's ratio;
  score                LM.score of a 100-hypothesis list: host time from the call to the synchronised result, median and min-max.

--leg pbert: the phone-to-word masked LM (modeling/p2w.py, lm_type="pbert") at the size of the reference's del_pc_mlm.yaml (d = 256,
4 + 4 layers, V = 10 872, 45 phones), bf16:
  step                 a full training step (30 % of the words masked, about three phones per word): us per step, tokens/s;
  correct_kernels      the correction step's kernels at T' = 300 frames, 40 tokens (row_lse + ctc_token_conf + correct_fuse) against
                       the same step composed from torch ops (softmax, gather, argmax) as alternating legs in ONE process;
  correct_step         host milliseconds per corrected utterance end to end (correct_step_timing below): T' = 300, 40 tokens.

--leg pelectra: P-ELECTRA (modeling/pelectra.py) with the pbert leg's generator and the electra leg's discriminator, batch 100, bf16,
dropout 0.1:
  step                 a full training step (train_lm.train_step) with the sampling head in the product's epilogue
                       (PELECTRA.sample_head = "fused") against the materialised logits of the labelled rows + sample_rows
                       ("materialised"), as alternating legs of --steps steps after --warmup in ONE process, --pairs pairs: ms per
                       step as median and range, every pair's ratio, torch.cuda.max_memory_allocated of each path;
  all_rows             the reference's shape of the generator's head alone on the same batch: logits of ALL B * L rows
                       (cmlm_head(want_logits=True)) followed by sample_rows over them -- the head's time and peak memory, next to
                       the two heads above timed alone.
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

LM12 = dict(lm_type="transformer", vocab_size=10000, hidden_size=256, num_layers=12, num_attention_heads=4,
            intermediate_size=1024, max_seq_len=256)     # bench.py: LM12


def libri_like_batch(batch, vocab, seed=0):
    """next-token batch with sentence lengths like LibriSpeech transcripts in a 10 k word-piece vocabulary (median ~40 tokens,
    a tail to ~120)"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.exp(torch.randn(batch, generator=g) * 0.55 + 3.65).clamp(4, 160).to(torch.int64).tolist()
    N = max(lens)
    ys = torch.full((batch, N), 2, dtype=torch.int64)
    labels = torch.full((batch, N), -100, dtype=torch.int64)
    for b, n in enumerate(lens):
        y = torch.randint(3, vocab, (n + 1,), generator=g)
        ys[b, :n], labels[b, :n] = y[:-1], y[1:]
    return {"ys_in": ys, "ylens": torch.tensor(lens), "labels": labels}, sum(lens)


def mlm_batch(batch, vocab, mask_id, proportion, seed=0):
    """the lengths of libri_like_batch; max(int(n * proportion), 1) positions of every row masked and labelled"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.exp(torch.randn(batch, generator=g) * 0.55 + 3.65).clamp(4, 160).to(torch.int64).tolist()
    N = max(lens)
    ys = torch.full((batch, N), 2, dtype=torch.int64)
    for b, n in enumerate(lens):
        ys[b, :n] = torch.randint(3, mask_id, (n,), generator=g)
    ys_in, labels = ys.clone(), torch.full((batch, N), -100, dtype=torch.int64)
    for b, n in enumerate(lens):
        for j in torch.randperm(n, generator=g)[: max(int(n * proportion), 1)].tolist():
            labels[b, j], ys_in[b, j] = ys[b, j], mask_id
    return {"ys": ys, "ys_in": ys_in, "ylens": torch.tensor(lens), "labels": labels}, sum(lens)


def bert_leg(args):
    import time
    from emoasr_amd.modeling.lm import LM
    from emoasr_amd.optimizers import AdamW, ScheduledOptimizer, get_optimizer_params_nodecay
    from emoasr_amd.train_lm import train_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    V = LM12["vocab_size"]
    params = SimpleNamespace(**dict(LM12, lm_type="bert", mask_id=V - 1, learning_rate=1e-4, lr_schedule_type="lindecay",
                                    num_warmup_steps=100, weight_decay=0.01, clip_grad_norm=1.0, accum_grad=1, log_step=10 ** 9))
    lm = LM(params, compute_dtype=torch.bfloat16).to(dev)
    out = {"leg": "bert", "batch": args.batch, "dtype": "bf16"}
    # ---- (a) pseudo-log-likelihood of an N-best list
    data, tokens = mlm_batch(args.batch, V, V - 1, 0.15)
    N = int(data["ylens"].max())
    Np = min((N + 7) // 8 * 8, LM12["max_seq_len"])
    lm.eval()
    out["score"] = {"hypotheses": args.batch, "copies": tokens, "padded_length": Np, "token_rows": tokens * Np, "runs": []}
    for budget in args.token_rows:
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lm.masked_logprobs(data["ys"], data["ylens"], max_token_rows=budget)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        run()
        sec = statistics.median(run() for _ in range(args.pairs))
        out["score"]["runs"].append({"max_token_rows": budget, "chunks": -(-tokens // max(1, budget // Np)), "ms": round(sec * 1e3, 2),
                                     "copies_per_s": round(tokens / sec), "token_rows_per_s": round(tokens * Np / sec),
                                     "head_taken": lm.last_head})
    # ---- (b) the masked-LM training step: head on the labelled rows against head on all rows
    lm.train()
    opt = ScheduledOptimizer(AdamW(get_optimizer_params_nodecay(list(lm.named_parameters()), params.weight_decay), lr=0,
                                   weight_decay=params.weight_decay), params, num_total_steps=10 ** 6)
    out["mlm_step"] = []
    for proportion in (0.15, 0.3):
        data, tokens = mlm_batch(args.batch, V, V - 1, proportion)
        step = lambda: train_step(lm, opt, data, params, dev, sync=False)
        rec = {"mask_proportion": proportion, "tokens": tokens, "rows_padded": data["ys_in"].numel(),
               "rows_labelled": int((data["labels"] != -100).sum()), "labelled_us": [], "all_rows_us": []}
        for _ in range(args.pairs):
            for at_labels in (True, False):
                lm.head_at_labels = at_labels
                timed(step, args.warmup)
                rec["labelled_us" if at_labels else "all_rows_us"].append(round(timed(step, args.steps), 1))
                rec["head_taken_labelled" if at_labels else "head_taken_all_rows"] = lm.last_head
        rec["pair_ratio_labelled_over_all_rows"] = [round(a / b, 3) for a, b in zip(rec["labelled_us"], rec["all_rows_us"])]
        rec["tokens_per_s_labelled"] = round(tokens / statistics.median(rec["labelled_us"]) * 1e6)
        rec["tokens_per_s_all_rows"] = round(tokens / statistics.median(rec["all_rows_us"]) * 1e6)
        out["mlm_step"].append(rec)
    lm.head_at_labels = True
    print(json.dumps(out))


def electra_batch(batch, vocab, mask_id, num_to_mask, max_len, seed=0):
    """sequences of concatenated utterances (median ~120 tokens, 40 .. max_len), exactly num_to_mask positions of every row masked"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.exp(torch.randn(batch, generator=g) * 0.4 + 4.8).clamp(max(40, num_to_mask), max_len).to(torch.int64).tolist()
    N = max(lens)
    ys = torch.full((batch, N), 2, dtype=torch.int64)
    for b, n in enumerate(lens):
        ys[b, :n] = torch.randint(3, mask_id, (n,), generator=g)
    ys_in, labels = ys.clone(), torch.full((batch, N), -100, dtype=torch.int64)
    for b, n in enumerate(lens):
        for j in torch.randperm(n, generator=g)[:num_to_mask].tolist():
            labels[b, j], ys_in[b, j] = ys[b, j], mask_id
    return {"ys": ys, "ys_in": ys_in, "ylens": torch.tensor(lens), "labels": labels}, sum(lens)


def electra_leg(args):
    import time
    from emoasr_amd.modeling.lm import LM
    from emoasr_amd.optimizers import AdamW, ScheduledOptimizer, get_optimizer_params_nodecay
    from emoasr_amd.train_lm import train_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    V, batch, num_to_mask = 9798, 90, 35
    size = dict(embedding_size=256, hidden_size=256, intermediate_size=1024, num_attention_heads=4, num_layers=12)
    cfg = dict(lm_type="electra", vocab_size=V, max_seq_len=256, mask_id=V - 1, electra_disc_weight=50,
               **{f"{s}_{k}": v for s in ("gen", "disc") for k, v in size.items()})
    params = SimpleNamespace(**dict(cfg, learning_rate=1e-4, lr_schedule_type="lindecay", num_warmup_steps=100, weight_decay=0.01,
                                    clip_grad_norm=5.0, accum_grad=1, log_step=10 ** 9))
    lm = LM(params, compute_dtype=torch.bfloat16).to(dev).train()
    opt = ScheduledOptimizer(AdamW(get_optimizer_params_nodecay(list(lm.named_parameters()), params.weight_decay), lr=0,
                                   weight_decay=params.weight_decay), params, num_total_steps=10 ** 6)
    data, tokens = electra_batch(batch, V, V - 1, num_to_mask, 256)
    step = lambda: train_step(lm, opt, data, params, dev, sync=False)
    rec = {"tokens": tokens, "rows_padded": data["ys_in"].numel(), "rows_labelled": int((data["labels"] != -100).sum()),
           "hip_us": [], "torch_us": []}
    for _ in range(args.pairs):
        for path in ("hip", "torch"):
            lm.sample_path = path
            timed(step, args.warmup)
            rec[path + "_us"].append(round(timed(step, args.steps), 1))
    lm.sample_path = "hip"
    for path in ("hip", "torch"):
        us = rec[path + "_us"]
        rec[path + "_median_us"], rec[path + "_min_max_us"] = statistics.median(us), [min(us), max(us)]
        rec["tokens_per_s_" + path] = round(tokens / statistics.median(us) * 1e6)
    rec["pair_ratio_hip_over_torch"] = [round(a / b, 4) for a, b in zip(rec["hip_us"], rec["torch_us"])]
    out = {"leg": "electra", "batch": batch, "dtype": "bf16", "step": rec}
    # ---- N-best scoring: one discriminator pass per list
    hyps, _ = mlm_batch(100, V, V - 1, 0.15, seed=1)
    lm.eval()

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lm.score(hyps["ys"], hyps["ylens"])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    run()
    ms = [run() for _ in range(max(args.pairs, 5))]
    out["score"] = {"hypotheses": 100, "tokens": int(hyps["ylens"].sum()), "padded_length": int(hyps["ys"].shape[1]),
                    "median_ms": round(statistics.median(ms), 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)]}
    print(json.dumps(out))


def pbert_leg(args):
    """the phone-to-word masked LM at the size of the reference's asr/correct/exps/csj/del_pc_mlm.yaml, and the correction kernels"""
    from emoasr_amd import ops
    from emoasr_amd.modeling.p2w import P2W
    from emoasr_amd.optimizers import AdamW, ScheduledOptimizer, get_optimizer_params_nodecay
    from emoasr_amd.train_lm import train_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    V, PV = 10872, 45
    cfg = dict(lm_type="pbert", input_layer="embed", enc_hidden_size=256, enc_num_attention_heads=4, enc_num_layers=4,
               enc_intermediate_size=1024, dec_hidden_size=256, dec_num_attention_heads=4, dec_num_layers=4,
               dec_intermediate_size=1024, dropout_enc_rate=0.1, dropout_dec_rate=0.1, dropout_attn_rate=0.1, mtl_ctc_weight=0,
               lsm_prob=0, kd_weight=0, max_decode_ylen=256, vocab_size=V, src_vocab_size=PV, max_seq_len=256, eos_id=2,
               mask_id=V - 1, phone_eos_id=2, phone_mask_id=PV - 2, blank_id=0, add_sos_eos=False)
    params = SimpleNamespace(**dict(cfg, learning_rate=1e-4, lr_schedule_type="lindecay", num_warmup_steps=100, weight_decay=0.01,
                                    clip_grad_norm=5.0, accum_grad=1, log_step=10 ** 9))
    lm = P2W(params, compute_dtype=torch.bfloat16).to(dev).train()
    opt = ScheduledOptimizer(AdamW(get_optimizer_params_nodecay(list(lm.named_parameters()), params.weight_decay), lr=0,
                                   weight_decay=params.weight_decay), params, num_total_steps=10 ** 6)
    data, tokens = mlm_batch(args.batch, V, V - 1, 0.3)
    g = torch.Generator().manual_seed(1)
    plens = (data["ylens"] * 3).clamp(max=256)      # about three phones per word
    data["plens"] = plens
    data["ps"] = torch.randint(3, PV - 2, (args.batch, int(plens.max())), generator=g)
    step = lambda: train_step(lm, opt, data, params, dev, sync=False)
    timed(step, args.warmup)
    us = [round(timed(step, args.steps), 1) for _ in range(args.pairs)]
    out = {"leg": "pbert", "batch": args.batch, "dtype": "bf16",
           "step": {"tokens": tokens, "phones": int(plens.sum()), "rows_labelled": int((data["labels"] != -100).sum()), "us": us,
                    "median_us": statistics.median(us), "tokens_per_s": round(tokens / statistics.median(us) * 1e6)}}
    # ---- the correction kernels at T' = 300 frames, 40 tokens, against the same step composed from torch ops
    T, n, Va = 300, 40, V
    best = torch.zeros(1, T, dtype=torch.int32)
    best[0, 2:T:7] = torch.randint(1, Va, (len(range(2, T, 7)),), generator=g, dtype=torch.int32)[: len(range(2, T, 7))]
    best[0, 3:T:7] = best[0, 2:T:7][: len(range(3, T, 7))]
    ntok = len(range(2, T, 7))
    n = min(n, ntok)
    logits = torch.randn(1, T, Va, generator=g).to(dev)
    lm_logits = torch.randn(n, V, generator=g).to(dev).to(torch.bfloat16)
    best_d, el = best.to(dev), torch.tensor([T], dtype=torch.int32, device=dev)

    def hip():
        lse = ops.row_lse(logits.view(T, Va))
        frame, conf, _ = ops.ctc_token_conf(logits, lse, best_d, el, 0)
        return ops.correct_fuse(logits.view(T, Va), lse, lm_logits, 0.5, Va, asr_rows=frame.view(-1)[:n])

    tok_frames = torch.tensor(list(range(2, T, 7))[:n], device=dev)
    tok_ids = best_d[0, tok_frames].long()

    def composed():     # soft-max of every frame, gather, the two frames of a run compared, gather, soft-max, mix, arg-max
        p = torch.softmax(logits[0], dim=-1)
        two = torch.stack([p[tok_frames, tok_ids], p[tok_frames + 1, tok_ids]])
        fr = tok_frames + two.argmax(dim=0)
        mix = 0.5 * p[fr] + 0.5 * torch.softmax(lm_logits.float(), dim=-1)[:, :Va]
        return mix.argmax(dim=-1), mix.max(dim=-1).values

    a, b = hip(), composed()
    assert torch.equal(a[0].long(), b[0]), "the kernels and the composed step disagree"
    rec = {"frames": T, "tokens": n, "V": Va, "hip_us": [], "torch_us": []}
    for _ in range(args.pairs):
        for name, fn in (("hip", hip), ("torch", composed)):
            timed(fn, args.warmup)
            rec[name + "_us"].append(round(timed(fn, args.steps), 1))
    rec["hip_median_us"], rec["torch_median_us"] = statistics.median(rec["hip_us"]), statistics.median(rec["torch_us"])
    rec["pair_ratio_hip_over_torch"] = [round(x / y, 3) for x, y in zip(rec["hip_us"], rec["torch_us"])]
    out["correct_kernels"] = rec
    out["correct_step"] = correct_step_timing(args, lm.eval(), V, PV, dev)
    print(json.dumps(out))


def pelectra_leg(args):
    from emoasr_amd import ops
    from emoasr_amd.modeling.pelectra import PELECTRA
    from emoasr_amd.optimizers import AdamW, ScheduledOptimizer, get_optimizer_params_nodecay
    from emoasr_amd.train_lm import train_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    V, PV = 10872, 45
    disc = dict(embedding_size=256, hidden_size=256, intermediate_size=1024, num_attention_heads=4, num_layers=12)
    cfg = dict(lm_type="pelectra", input_layer="embed", enc_hidden_size=256, enc_num_attention_heads=4, enc_num_layers=4,
               enc_intermediate_size=1024, dec_hidden_size=256, dec_num_attention_heads=4, dec_num_layers=4,
               dec_intermediate_size=1024, dropout_enc_rate=0.1, dropout_dec_rate=0.1, dropout_attn_rate=0.1, mtl_ctc_weight=0,
               lsm_prob=0, kd_weight=0, max_decode_ylen=256, vocab_size=V, src_vocab_size=PV, max_seq_len=256, eos_id=2,
               mask_id=V - 1, phone_eos_id=2, phone_mask_id=PV - 2, blank_id=0, add_sos_eos=False, electra_disc_weight=50,
               **{f"disc_{k}": v for k, v in disc.items()})
    params = SimpleNamespace(**dict(cfg, learning_rate=1e-4, lr_schedule_type="lindecay", num_warmup_steps=100, weight_decay=0.01,
                                    clip_grad_norm=5.0, accum_grad=1, log_step=10 ** 9))
    lm = PELECTRA(params, compute_dtype=torch.bfloat16).to(dev).train()
    opt = ScheduledOptimizer(AdamW(get_optimizer_params_nodecay(list(lm.named_parameters()), params.weight_decay), lr=0,
                                   weight_decay=params.weight_decay), params, num_total_steps=10 ** 6)
    data, tokens = mlm_batch(args.batch, V, V - 1, 0.3)
    g = torch.Generator().manual_seed(1)
    plens = (data["ylens"] * 3).clamp(max=256)      # about three phones per word
    data["plens"] = plens
    data["ps"] = torch.randint(3, PV - 2, (args.batch, int(plens.max())), generator=g)
    step = lambda: train_step(lm, opt, data, params, dev, sync=False)
    heads = ("fused", "materialised")
    rec = {"tokens": tokens, "phones": int(plens.sum()), "rows_padded": data["ys_in"].numel(),
           "rows_labelled": int((data["labels"] != -100).sum()), "fused_ms": [], "materialised_ms": []}
    for _ in range(args.pairs):
        for head in heads:
            lm.sample_head = head
            timed(step, args.warmup)
            torch.cuda.reset_peak_memory_stats()
            rec[head + "_ms"].append(round(timed(step, args.steps) / 1e3, 3))
            rec[head + "_peak_bytes"] = torch.cuda.max_memory_allocated()
            rec[head + "_head_taken"] = lm.last_head
    for head in heads:
        ms = rec[head + "_ms"]
        rec[head + "_median_ms"], rec[head + "_min_max_ms"] = statistics.median(ms), [min(ms), max(ms)]
    rec["pair_ratio_fused_over_materialised"] = [round(a / b, 4) for a, b in zip(rec["fused_ms"], rec["materialised_ms"])]
    out = {"leg": "pelectra", "batch": args.batch, "dtype": "bf16", "step": rec}
    # ---- the generator's head alone on this batch's hidden rows: the two heads above and the reference's all-rows shape
    eng = lm.engine()
    B, L = data["ys_in"].shape
    x = torch.randn(B * L, 256, device=dev).to(torch.bfloat16)
    valid = (data["labels"] != -100).view(-1)
    sel = valid.nonzero().view(-1).to(dev)
    lab = data["labels"].view(-1)[valid].to(torch.int32).to(dev)
    w = torch.full((sel.numel(),), 1.0 / sel.numel(), device=dev)
    lab_all, w_all = data["labels"].clamp(min=0).to(torch.int32).view(-1).to(dev), valid.float().to(dev)

    def head(fused):
        return lambda: eng.cmlm_head(x, sel, lab, w, False, False, sample_seed=7, sample_fused=fused)

    def all_rows():
        _, _, logits = eng.cmlm_head(x, sel, lab, w, False, True)
        ops.sample_rows(logits, lab_all, w_all, 7)

    hrec = {"rows_all": B * L}
    for name, fn in (("fused", head(True)), ("materialised", head(False)), ("all_rows", all_rows)):
        timed(fn, 3)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        us = [round(timed(fn, 10), 1) for _ in range(args.pairs)]
        hrec[name + "_us"], hrec[name + "_median_us"] = us, statistics.median(us)
        hrec[name + "_peak_bytes_above_resident"] = torch.cuda.max_memory_allocated() - base
    out["head_alone"] = hrec
    print(json.dumps(out))


def correct_step_timing(args, lm, V, PV, dev):
    """host milliseconds per corrected utterance (correct.correct_step: encoder pass, both heads, greedy paths, confidences, one copy,
    the LM forward, the fusion, one copy) with the 23 M Conformer-CTC of bench.py plus a hierarchical phone head, bf16, on 1 203
    input frames = T' = 300.  The weights are random: the word head is sharpened and the blank's bias is bisected until the greedy
    hypothesis has 40 tokens (or as near as the bisection gets: the count is reported)."""
    import time
    from emoasr_amd.correct import correct_step
    from emoasr_amd.modeling.asr import ASR
    cfg = dict(input_layer="conv2d", feat_dim=80, num_framestacks=1, encoder_type="conformer", decoder_type="ctc",
               pos_encode_type="rel", enc_hidden_size=256, enc_num_attention_heads=4, enc_num_layers=12, enc_intermediate_size=1024,
               dropout_enc_rate=0.1, dropout_attn_rate=0.1, vocab_size=V, blank_id=0, eos_id=2, kd_weight=0,
               mtl_phone_ctc_weight=0.3, hie_mtl_phone=True, phone_vocab_size=PV, inter_ctc_layer_id=6)
    torch.manual_seed(2)
    asr = ASR(SimpleNamespace(**cfg), phase="test", compute_dtype=torch.bfloat16).to(dev).eval()
    xs = torch.randn(1, 1203, 80)
    data = {"utt_ids": ["utt"], "xs": xs, "xlens": torch.tensor([1203]), "texts": [""]}
    with torch.no_grad():
        asr.decoder.output.weight.mul_(20.0)
        asr.decoder.phone_output.weight.mul_(20.0)
        lo, hi = -2000.0, 2000.0
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            asr.decoder.output.bias[0] = mid
            n = len(asr.decode(xs.to(dev), data["xlens"])[0][0])
            if n == 40:
                break
            lo, hi = (mid, hi) if n > 40 else (lo, mid)
    det = {}
    step = lambda: correct_step(asr, lm, data, 0, V - 1, 0.9, 0.5, dev, V, details=det)
    _, hyp, _, _, num_masked, num_tokens = step()

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for _ in range(args.warmup):
        run()
    ms = [run() for _ in range(max(args.steps, 5))]
    return {"frames": 300, "tokens": num_tokens, "phones": int(len(det["hyp_phone"])), "masked": num_masked, "lm": "pbert",
            "median_ms": round(statistics.median(ms), 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)]}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3     # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--leg", choices=["transformer", "bert", "electra", "pbert", "pelectra"], default="transformer")
    ap.add_argument("--token-rows", type=int, nargs="+", default=[16384, 65536, 262144], help="--leg bert: max_token_rows values")
    args = ap.parse_args()
    if args.leg == "bert":
        return bert_leg(args)
    if args.leg == "electra":
        return electra_leg(args)
    if args.leg == "pbert":
        return pbert_leg(args)
    if args.leg == "pelectra":
        return pelectra_leg(args)
    from emoasr_amd import ops
    from emoasr_amd.modeling.lm import LM
    from emoasr_amd.optimizers import AdamW, ScheduledOptimizer, get_optimizer_params_nodecay
    from emoasr_amd.train_lm import train_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    params = SimpleNamespace(**dict(LM12, learning_rate=1e-4, lr_schedule_type="lindecay", num_warmup_steps=100, weight_decay=0.01,
                                    clip_grad_norm=1.0, accum_grad=1, log_step=10 ** 9))
    lm = LM(params, compute_dtype=torch.bfloat16).to(dev).train()
    opt = ScheduledOptimizer(AdamW(get_optimizer_params_nodecay(list(lm.named_parameters()), params.weight_decay), lr=0,
                                   weight_decay=params.weight_decay), params, num_total_steps=10 ** 6)
    data, tokens = libri_like_batch(args.batch, LM12["vocab_size"])
    rows = data["ys_in"].numel()
    out = {"batch": args.batch, "tokens": tokens, "rows_padded": rows, "dtype": "bf16"}
    step = lambda: train_step(lm, opt, data, params, dev, sync=False)
    for fused in (True, False, True, False):
        lm.fused_head = fused
        timed(step, args.warmup)
        us = timed(step, args.steps)
        key = "train_tokens_per_s" if fused else "train_tokens_per_s_materialised"
        out.setdefault(key, []).append(round(tokens / us * 1e6))
        out["head_taken" if fused else "head_taken_materialised"] = lm.last_head
    # ---- the head alone on the same rows
    d, V = LM12["hidden_size"], LM12["vocab_size"]
    x = torch.randn(rows, d, device=dev).to(torch.bfloat16)
    w = (torch.randn(V, d, device=dev) * 0.1).to(torch.bfloat16)
    bias = torch.zeros(V, device=dev)
    lab = data["labels"].clamp(min=0).to(torch.int32).view(-1).to(dev)
    wrow = ((data["labels"] != -100).float() / tokens).view(-1).to(dev)
    dw, db = torch.zeros(V, d, device=dev), torch.zeros(V, device=dev)

    def fused_head():
        _, _, ctx = ops.ce_head_fwd(x, w, bias, lab, wrow)
        ops.ce_head_bwd(x, w, bias, ctx, dw, db)

    def materialised_head():
        logits, _ = ops.gemm_nt_lse(x, w, bias)
        _, dz = ops.lsm_loss(logits, lab, wrow, 0.0, True)
        ops.gemm_tn(dz, x, out=dw, accumulate=True, colsum=db)
        ops.gemm_nn(dz, w)

    out["head_fused_ok"] = bool(ops.ce_head_ok(x, w))
    fu, ma = [], []
    timed(fused_head, 3), timed(materialised_head, 3)
    for _ in range(args.pairs):
        fu.append(timed(fused_head, 10))
        ma.append(timed(materialised_head, 10))
    out["head_fused_us"], out["head_materialised_us"] = round(statistics.median(fu), 1), round(statistics.median(ma), 1)
    out["head_pair_ratio_fused_over_materialised"] = [round(a / b, 3) for a, b in zip(fu, ma)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
