"""LM training and evaluation drivers with the reference's semantics (lm/train_lm.py:40-130, lm/test_ppl.py:32-74), for the
Transformer LM (modeling/lm.py), the RNN LM (lm_type="rnn", modeling/rnnlm.py), the BERT masked LM (lm_type="bert",
modeling/lm.py) and ELECTRA (lm_type="electra" / "electra-disc", modeling/lm.py) alike -- all are `LM(params)` and take `(ys_in, ylens, labels)`; the causal ones expose `token_logprobs` for the
perplexity (ppl_lm), the masked one `masked_logprobs` (ppl_masked_lm):

    model = LM(params, compute_dtype=...).cuda().train()
    groups = get_optimizer_params_nodecay(list(model.named_parameters()), weight_decay=params.weight_decay)
    optimizer = ScheduledOptimizer(AdamW(groups, lr=0, weight_decay=params.weight_decay), params, num_total_steps=...)
    for epoch in range(...):
        train(model, optimizer, dataloader, params, device, epoch)
        save(model, optimizer, save_dir, epoch + 1)

With `emoasr_amd.optimizers.AdamW` underneath, the gradient norm, the clip to params.clip_grad_norm, the NaN / Inf skip and the
update are the fused HIP step (one norm launch + one update launch, no host round trip); skipped updates are folded out of the
schedule position at the log-step synchronisation and at epoch boundaries, as emoasr_amd.train does.  With any torch optimizer
the reference's sequence runs literally.
"""
import logging
import math
import os

import torch

from . import checkpoint


def train_step(model, optimizer, data, params, device, no_grad=False, empty_cache=False, sync=True):
    """One micro-batch (lm/train_lm.py:40-84): forward, loss / accum_grad, backward; unless `no_grad` (still accumulating): clip,
    skip on a NaN gradient norm, step, zero_grad.  -> loss_dict of floats / accum_grad (sync=False: 0-dim device tensors); ELECTRA's
    per-utterance counts `num_replaced` / `num_masked` go through the same division, so logging stays one code path.
    A batch that carries `error_labels` (LMDataset for lm_type="electra-disc") goes to model.forward_disc, the discriminator-only
    step; the reference's driver never calls forward_disc (its electra-disc batches have no `labels` and fail there)."""
    from .optimizers import Adam as HipAdam
    if "error_labels" in data:
        loss, loss_dict = model.forward_disc(data["ys_in"], data["ylens"], data["error_labels"])
    else:
        loss, loss_dict = model(data["ys_in"], data["ylens"], data["labels"], data.get("ps"), data.get("plens"))
    accum = params.accum_grad
    loss_dict = {k: (v.item() / accum if sync else v.detach() / accum) for k, v in loss_dict.items()}
    (loss / accum).backward()
    if not no_grad:
        base = getattr(optimizer, "optimizer", optimizer)
        if isinstance(base, HipAdam):
            base.clip_grad_norm, base.grad_mult = params.clip_grad_norm, 1.0
            optimizer.step()
        else:
            grad_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), params.clip_grad_norm)
            if math.isnan(grad_norm):
                logging.warning("do not update because of nan grad_norm")
            else:
                optimizer.step()
        optimizer.zero_grad()
        if empty_cache:
            torch.cuda.empty_cache()
    return loss_dict


def train(model, optimizer, dataloader, params, device, epoch, empty_cache=False, log=None):
    """One epoch (lm/train_lm.py:87-130): every accum_grad-th micro-batch steps the optimizer; the running loss sums are logged
    every params.log_step optimizer steps -- the loop's only host synchronisation.  -> optimizer steps taken"""
    log = log or logging.info
    optimizer.update_epoch()
    step, sums = 0, {}
    n_total = len(dataloader) // params.accum_grad if hasattr(dataloader, "__len__") else -1
    for accum_step, data in enumerate(dataloader):
        stepping = (accum_step + 1) % params.accum_grad == 0
        loss_dict = train_step(model, optimizer, data, params, device, no_grad=not stepping,
                               empty_cache=empty_cache and stepping, sync=False)
        step += int(stepping)
        for k, v in loss_dict.items():
            sums[k] = sums[k] + v if k in sums else v
        if stepping and step % params.log_step == 0:
            if hasattr(optimizer, "fold_skipped"):
                optimizer.fold_skipped()
            detail = " ".join(f"{k}: {float(v) / params.log_step:.3f}" for k, v in sums.items())
            log(f"epoch = {(epoch + 1):>2} step = {step:>6} / {n_total:>6} lr = {optimizer._lr:.5f} " + detail)
            sums = {}
    return step


def save(model, optimizer, save_dir, epoch):
    """`model.ep{N}` / `optim.ep{N}` in the reference's formats (lm/train_lm.py:300-312) -> (model path, optimizer path)"""
    model_path, optim_path = os.path.join(save_dir, f"model.ep{epoch:d}"), os.path.join(save_dir, f"optim.ep{epoch:d}")
    checkpoint.save_model(model, model_path)
    torch.save(optimizer.state_dict(), optim_path)
    return model_path, optim_path


def resume(model, optimizer, save_dir, epoch=0):
    """load the latest (or the given) epoch's pair of files -> the epoch to continue from (0: nothing found)"""
    model_path, optim_path, epoch = checkpoint.resume_paths(save_dir, epoch)
    if epoch:
        checkpoint.load_model(model, model_path)
        optimizer.load_state_dict(torch.load(optim_path, map_location="cpu", weights_only=False))
    return epoch


def ppl_lm(dataloader, model, device, add_sos_eos=False):
    """lm/test_ppl.py:32-74: token-level perplexity over a loader of single utterances (LMDataset phase "test") -> (cnt, ppl).
    With add_sos_eos the first token's and the <eos> prediction are left out.  Built on the model's row log-probabilities
    (LM.token_logprobs: no [N, V] soft-max leaves the device), summed on the host in double precision."""
    cnt, sum_logprob = 0, 0.0
    for data in dataloader:
        ys = data["ys_in"]
        assert ys.size(0) == 1
        if ys.size(1) <= 1 or (add_sos_eos and ys.size(1) <= 3):
            logging.warning(f"skip {data['utt_ids'][0]}")
            continue
        ys_in, labels = ys[:, :-1], ys[:, 1:].clone()
        if add_sos_eos:
            labels[:, 0] = -100
            labels[:, -1] = -100
        lp = model.token_logprobs(ys_in, [int(data["ylens"][0]) - 1], labels)
        sum_logprob -= float(lp.sum())
        cnt += int((labels != -100).sum())
    return cnt, math.exp(sum_logprob / cnt)


def ppl_masked_lm(dataloader, model, device, mask_id=None, max_seq_len=None):
    """lm/test_ppl.py:77-133: masked-LM perplexity over a loader of single utterances (LMDataset phase "test") -> (cnt, ppl): every
    position of ys_in is masked in turn (the <eos> wrappers of add_sos_eos included) and predicted from the rest; an utterance
    longer than max_seq_len is skipped with a warning.  Built on LM.masked_logprobs (the copies are made on the device, one
    device-to-host copy per utterance), summed on the host in double precision.  mask_id / max_seq_len default to the model's.
    A P2W (lm_type "pbert", batches of P2WDataset) is scored the same way with the utterance's phones passed through."""
    if mask_id is not None:
        assert int(mask_id) == int(getattr(model, "mask_id", model.params.mask_id)), "mask_id differs from the model's"
    max_seq_len = model.params.max_seq_len if max_seq_len is None else max_seq_len
    cnt, sum_logprob = 0, 0.0
    for data in dataloader:
        ys = data["ys_in"]
        assert ys.size(0) == 1
        if ys.size(1) > max_seq_len:
            logging.warning(f"input length longer than {max_seq_len:d} skip")
            continue
        if hasattr(model, "masked_logprobs"):
            lp = model.masked_logprobs(ys, [int(data["ylens"][0])])
        else:      # a P2W "pbert": the N masked copies as one batch, every copy conditioned on the utterance's phones
            n = ys.size(1)
            copies = ys.repeat(n, 1)
            copies[torch.arange(n), torch.arange(n)] = int(model.params.mask_id)
            ps = data["ps"][:, : int(data["plens"][0])].repeat(n, 1)
            logp = torch.log_softmax(model(copies, ps=ps).float(), dim=-1).cpu()
            lp = logp[torch.arange(n), torch.arange(n), ys[0]]
        sum_logprob -= float(lp.sum())
        cnt += ys.size(1)
    return cnt, math.exp(sum_logprob / cnt)
