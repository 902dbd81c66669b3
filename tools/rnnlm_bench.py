"""The RNN LM at the size the reference's 13-14 M-parameter RNN LMs imply (E = H = 512, L = 2, V = 10000, bf16):

  step      one shallow-fusion step for nb hypotheses, the kernel (csrc/rnnlm.hip, L + 2 launches) against the chain of entry points
            that predate it (RNNLanguageModel._step_chain) -- same process, alternated, warmed up, device events around `--iters`
            consecutive steps (so the figure includes the launch sequencing a search pays), `--repeats` windows each: median, min,
            max; the two forms' log-probabilities are compared on the same inputs
  train     tokens/s of train_lm.train_step (forward, backward, fused AdamW) at B = 128, N = 64
  ctc_beam  real-time factor of the CTC prefix beam search on the ctcbeam_tiny utterances (10 ms frames) with this LM's family and
            with a Transformer LM of the same width (vocabulary 40: the acoustic model's)

    python tools/rnnlm_bench.py [--nb 1 10 16 32] [--iters 200] [--repeats 7] [--skip-train] [--skip-beam]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CFG = dict(lm_type="rnn", vocab_size=10000, embedding_size=512, hidden_size=512, num_layers=2, dropout_rate=0.1, tie_weights=False)


def _lm(cfg, dev, dtype=torch.bfloat16):
    from emoasr_amd.modeling.lm import LM
    torch.manual_seed(0)
    return LM(SimpleNamespace(**cfg), compute_dtype=dtype).to(dev)


def _stats(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 2), round(ts[0], 2), round(ts[-1], 2)]


def bench_step(dev, nbs, iters, repeats):
    lm = _lm(CFG, dev).eval()
    V = CFG["vocab_size"]
    for nb in nbs:
        pools = lm.new_pools(2 * nb, nb)
        g = torch.Generator().manual_seed(nb)
        pools.ph.copy_(torch.randn(pools.ph.shape, generator=g).mul(0.5))
        pools.pc.copy_(torch.randn(pools.pc.shape, generator=g))
        ph0, pc0 = pools.ph.clone(), pools.pc.clone()
        ids = torch.randint(0, V, (nb,), generator=g).to(torch.int32).to(dev)
        # a search's pattern: the parents in one half of the pool, the children in the other, halves swapped every step
        ctl = [(torch.arange(nb, dtype=torch.int32, device=dev) + a, torch.arange(nb, dtype=torch.int32, device=dev) + b)
               for a, b in ((0, nb), (nb, 0))]

        def run(kernel, n):
            lm.step_kernel = kernel
            for i in range(n):
                lm.step(pools, nb, ids, ctl[i % 2][0], ctl[i % 2][1])

        out = {}
        for kernel in (True, False):      # same inputs, one step: the two forms' results
            pools.ph.copy_(ph0)
            pools.pc.copy_(pc0)
            run(kernel, 1)
            out[kernel] = (pools.logp.clone(), pools.ph.clone())
            assert lm.last_step == ("kernel" if kernel else "chain")
        times = {True: [], False: []}
        for kernel in (True, False):
            run(kernel, 20)     # warm-up of both forms at this shape
        torch.cuda.synchronize()
        for _ in range(repeats):
            for kernel in (True, False):     # alternated windows
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(kernel, iters)
                e1.record()
                torch.cuda.synchronize()
                times[kernel].append(e0.elapsed_time(e1) * 1e3 / iters)
        k, c = _stats(times[True]), _stats(times[False])
        print(json.dumps(dict(bench="step", nb=nb, iters=iters, repeats=repeats, kernel_us=k, chain_us=c,
                              chain_over_kernel=round(c[0] / k[0], 2),
                              max_logp_diff=round((out[True][0] - out[False][0]).abs().max().item(), 4),
                              max_h_diff=round((out[True][1].float() - out[False][1].float()).abs().max().item(), 4))), flush=True)


def bench_train(dev, B=128, N=64, iters=10):
    from emoasr_amd.optimizers import AdamW, ScheduledOptimizer, get_optimizer_params_nodecay
    from emoasr_amd.train_lm import train_step
    params = SimpleNamespace(**dict(CFG, learning_rate=1e-3, lr_schedule_type="lindecay", num_warmup_steps=2, weight_decay=0.01,
                                    clip_grad_norm=5.0, accum_grad=1, log_step=1))
    lm = _lm(CFG, dev).train()
    groups = get_optimizer_params_nodecay(list(lm.named_parameters()), weight_decay=params.weight_decay)
    opt = ScheduledOptimizer(AdamW(groups, lr=0, weight_decay=params.weight_decay), params, num_total_steps=1000)
    g = torch.Generator().manual_seed(2)
    y = torch.randint(3, CFG["vocab_size"], (B, N + 1), generator=g)
    batch = {"ys_in": y[:, :-1], "ylens": torch.full((B,), N), "labels": y[:, 1:]}
    for _ in range(3):
        train_step(lm, opt, batch, params, dev)
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        loss = train_step(lm, opt, batch, params, dev)["loss_total"]     # (.item(): the step ends in a device synchronise)
        ts.append(time.perf_counter() - t0)
    s = _stats([t * 1e3 for t in ts])
    print(json.dumps(dict(bench="train", B=B, N=N, step_ms=s, tokens_per_s=round(B * N / (s[0] * 1e-3)), head=lm.last_head,
                          loss=round(loss, 4))), flush=True)


def bench_ctc_beam(dev, repeats=3):
    from emoasr_amd.modeling.asr import ASR
    from tests.util import CONFIGS, load_ctc_beam_golden
    _, sd, _, g2, _ = load_ctc_beam_golden()
    model = ASR(SimpleNamespace(**CONFIGS["l2_tiny"]), compute_dtype=torch.bfloat16)
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    lms = {"rnn": _lm(dict(CFG, vocab_size=40), dev).eval(),
           "transformer": _lm(dict(lm_type="transformer", vocab_size=40, hidden_size=512, num_layers=2, num_attention_heads=8,
                                   intermediate_size=2048, max_seq_len=64), dev).eval()}
    utts = [(g2["xs"][b:b + 1, : int(g2["xlens"][b])].to(dev), g2["xlens"][b:b + 1]) for b in (0, 1, 2, 3)]
    audio_s = sum(int(xl[0]) for _, xl in utts) * 0.01
    for name, lm in lms.items():
        ts = []
        for r in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for x, xl in utts:
                model.decode(x, xl, beam_width=10, len_weight=0.1, lm=lm, lm_weight=0.3)
            torch.cuda.synchronize()
            if r:      # (the first pass warms up)
                ts.append(time.perf_counter() - t0)
        s = _stats([t * 1e3 for t in ts])
        print(json.dumps(dict(bench="ctc_beam", lm=name, beam_width=10, audio_s=round(audio_s, 2), decode_ms=s,
                              rtf=round(s[0] * 1e-3 / audio_s, 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, nargs="+", default=[1, 10, 16, 32])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--skip-beam", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    bench_step(dev, a.nb, a.iters, a.repeats)
    if not a.skip_train:
        bench_train(dev)
    if not a.skip_beam:
        bench_ctc_beam(dev)


if __name__ == "__main__":
    main()
