"""The LAS decoder (decoder_type "las": emoasr_amd/modeling/decoders/las.py, engine/las.py, csrc/las.hip) on the device against
the reference's values (tests/golden/las_tiny*.npz, written by tests/golden/make_golden_las.py) and against tests/las_ref.py.

Model bars are those of tests/test_p2w_gpu.py: loss 1e-3 (f32) / 2e-2 (bf16) relative, f32 gradients 5e-3 in the max-error form with
cosine >= 0.9999 per tensor, bf16 gradients cosine > 0.98 over the tensors above 1e-2 of the largest, f32 logits 1e-3 of their range,
bf16 logits 4 x the CPU-simulated bf16 error (LAS_LOGITS_BF16_SIM).  "f32x3" is held to the f32 bars.  The attention kernels are
held to 4 x the error that the float64 restatement itself makes in f32 torch on the CPU (KERNEL_F32_FLOOR)."""
from types import SimpleNamespace

import pytest
import torch

from tests import las_ref

pytestmark = pytest.mark.gpu

# the restatement in f32 against itself in f64 over the seeded kernel cases (T = 1, 37, 211, with and without lengths), largest error
# over every output and gradient in las_ref.step_errors' units: 5.98e-7 (tests/test_las_cpu.py::test_f32_kernel_floor_constant
# recomputes it).  Measured on the device: 3.3e-8 .. 7.8e-7 over these cases, dropout included.
KERNEL_F32_FLOOR = 5.98e-7
# tests/las_ref.py with matrices and stored activations rounded to bf16 against itself unrounded, valid positions, of the logits' range
# (tests/test_las_cpu.py::test_bf16_logit_error_constant recomputes both)
LAS_LOGITS_BF16_SIM = {"a": 2.976e-3, "b": 2.763e-3}
_MODES = [torch.float32, torch.bfloat16, "f32x3"]
_MODE_IDS = ["f32", "bf16", "f32x3"]


@pytest.fixture(scope="module")
def fx():
    return las_ref.load_las_golden()


def _model(fx, dev, mode, train=True, encoder=False, **over):
    from emoasr_amd.modeling.asr import ASR
    from tests.util import load_golden
    cfg, sd, _ = fx
    torch.manual_seed(0)
    model = ASR(SimpleNamespace(**dict(las_ref.las_asr_config(cfg), **over)), compute_dtype=mode)
    model.load_state_dict(sd, strict=False)
    if encoder:   # the l3_tiny encoder's weights live in that fixture
        _, sd3, _ = load_golden("l3_tiny")
        model.load_state_dict({k: v for k, v in sd3.items() if k.startswith("encoder.")}, strict=False)
    model.decoder.score.dropout_attn_rate = 0.0   # the goldens ran with every dropout at 0
    model = model.to(dev)
    return model.train() if train else model.eval()


def _run(model, g, case, dev, soft=None):
    eouts = g[f"{case}/eouts"].to(dev).requires_grad_(True)
    loss, ld, logits = model.decoder(eouts, g[f"{case}/elens"], None, g[f"{case}/ys"], g[f"{case}/ylens"], g[f"{case}/ys_in"],
                                     g[f"{case}/ys_out"], soft)
    loss.backward()
    return loss, ld, logits, eouts.grad


def _check_grads(model, g, case, mode, deouts):
    bf16 = mode == torch.bfloat16
    ref = {k[len(case) + 6:]: v for k, v in g.items() if k.startswith(case + "/grad/")}
    ref["eouts"] = g[f"{case}/deouts"]
    got = {n: p.grad for n, p in model.named_parameters() if n.startswith("decoder.")}
    got["eouts"] = deouts
    assert set(got) == set(ref)
    gmax = max(v.abs().max().item() for v in ref.values())
    worst, worst_name, cos_min, cos_name, big = 0.0, None, 1.0, None, 0
    for n, r in ref.items():
        x = got[n].float().cpu()
        assert torch.isfinite(x).all(), n
        err = ((x - r).abs().max() / max(r.abs().max().item(), 1e-2 * gmax)).item()
        if err > worst:
            worst, worst_name = err, n
        if r.abs().max() > (1e-2 if bf16 else 1e-6) * gmax:
            big += 1
            cos = torch.nn.functional.cosine_similarity(x.flatten().double(), r.flatten().double(), dim=0).item()
            if cos < cos_min:
                cos_min, cos_name = cos, n
    print(f"las {case} grads {mode}: worst max-error {worst:.3e} ({worst_name}), min cosine {cos_min:.8f} ({cos_name}) over {big} tensors")
    assert got["decoder.score.w_score.bias"].abs().max().item() == 0.0   # shift invariance: written as zero
    if bf16:
        # (not vacuous: 19 tensors of batch (a) and of the distillation case are above the threshold; in batch (b) the auxiliary
        # CTC loss over 211 frames dwarfs the attention loss, and its head's two tensors, w_score and the filter remain: 4)
        assert big >= 4 and cos_min > 0.98, (big, cos_min, cos_name, worst, worst_name)
        return
    assert worst < 5e-3, (worst, worst_name)
    assert cos_min >= 0.9999, (cos_min, cos_name)


def _check_losses(ld, g, case, mode, keys):
    ltol = 2e-2 if mode == torch.bfloat16 else 1e-3
    assert set(ld) == set(keys) | {"loss_total"}
    for k in ld:
        ref = g[f"{case}/{k}"].item()
        print(f"las {case} {k} {mode}: {ld[k].item():.6f} against {ref:.6f}")
        assert abs(ld[k].item() - ref) < ltol * abs(ref), (k, ld[k].item(), ref)


def _logit_error(logits, g, case):
    ref = g[f"{case}/logits"]
    ok = las_ref.valid_positions(g[f"{case}/ylens"], ref.shape[1])
    assert logits.shape == ref.shape
    return ((logits.float().cpu() - ref)[ok].abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("mode", _MODES, ids=_MODE_IDS)
@pytest.mark.parametrize("case", ["a", "b"])
def test_model_against_goldens(dev, fx, case, mode):
    g = fx[2]
    model = _model(fx, dev, mode)
    loss, ld, logits, deouts = _run(model, g, case, dev)
    assert ld["loss_total"] is loss
    _check_losses(ld, g, case, mode, ("loss_att", "loss_ctc"))
    err = _logit_error(logits, g, case)
    bar = 4 * LAS_LOGITS_BF16_SIM[case] if mode == torch.bfloat16 else 1e-3
    print(f"las {case} logits {mode}: {err:.3e} of range (bar {bar:.3e})")
    assert err <= bar, err
    _check_grads(model, g, case, mode, deouts)


@pytest.mark.parametrize("mode", _MODES[:2], ids=_MODE_IDS[:2])
def test_distillation_against_golden(dev, fx, mode):
    g = fx[2]
    model = _model(fx, dev, mode, kd_weight=0.5, reduce_main_loss_kd=False)
    loss, ld, logits, deouts = _run(model, g, "kd", dev, g["kd/soft"].to(dev))
    _check_losses(ld, g, "kd", mode, ("loss_att", "loss_ctc", "loss_kd"))
    _check_grads(model, g, "kd", mode, deouts)


# ---- the attention kernels against the float64 restatement ---------------------------------------------------------------------
def _device_step(T, ragged, dev, p=0.0, seed=0, step=0, dtype=torch.float32):
    from emoasr_amd import ops
    t, elens, dctx, daw = las_ref.kernel_case(T, ragged)
    d = {k: v.to(dev, dtype if k in ("pk", "pq", "eouts") else torch.float32).contiguous() for k, v in t.items()}
    W = ops.LasWeights(d["filt"], d["w_conv"], d["b_conv"], d["w_score"])
    el = None if elens is None else elens.to(dev, torch.int32)
    B, A, D = las_ref.KERNEL_B, las_ref.KERNEL_A, las_ref.KERNEL_D
    with ops.stream_scope(False):
        aw, ctx, lse = ops.las_attend_fwd(W, d["pk"], d["pq"], d["aw_prev"], d["eouts"], el, p, seed, step)
        z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        out = dict(aw=aw, ctx=ctx, dpq=z(B, A), daw_prev=z(B, T), dpk=z(B, T, A), deouts=z(B, T, D), dw_score=z(1, A), dw_conv=z(A, 10),
                   db_conv=z(A), dfilt=z(10, 1, 201))
        ops.las_attend_bwd(W, d["pk"], d["pq"], d["aw_prev"], d["eouts"], el, p, seed, step, aw, ctx, lse, dctx.to(dev, dtype),
                           daw.to(dev, torch.float32), out["dpq"], out["daw_prev"], out["dpk"], out["deouts"], out["dw_score"],
                           out["dw_conv"], out["db_conv"], out["dfilt"])
    torch.cuda.synchronize()
    return {k: v.float().cpu() for k, v in out.items()}


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("T", las_ref.KERNEL_T)
def test_attend_kernels_against_f64(dev, T, ragged):
    got = _device_step(T, ragged, dev)
    errs = las_ref.step_errors(got, las_ref.step_in_dtype(T, ragged, torch.float64))
    worst = max(errs, key=errs.get)
    print(f"las_attend T={T} ragged={ragged}: worst {errs[worst]:.3e} ({worst}); bar {4 * KERNEL_F32_FLOOR:.3e}")
    assert errs[worst] <= 4 * KERNEL_F32_FLOOR, errs


@pytest.mark.parametrize("T", [37, 211])
def test_attend_dropout_matches_the_exported_mask(dev, T):
    """forward and backward derive the mask las_dropmask exports: both equal the restatement fed that mask, at the kernel bars"""
    from emoasr_amd import ops
    p, seed, step = 0.1, 0xABCDEF, 3
    keep = ops.las_dropmask(las_ref.KERNEL_B, T, p, seed, step, dev).cpu()
    assert 0 < keep.sum() < keep.numel()
    got = _device_step(T, True, dev, p, seed, step)
    errs = las_ref.step_errors(got, las_ref.step_in_dtype(T, True, torch.float64, keep.double(), p))
    worst = max(errs, key=errs.get)
    print(f"las_attend dropout T={T}: worst {errs[worst]:.3e} ({worst}); bar {4 * KERNEL_F32_FLOOR:.3e}")
    assert errs[worst] <= 4 * KERNEL_F32_FLOOR, errs
    dropped = keep == 0
    assert dropped.any() and not got["aw"][dropped].any()


def test_dropmask_statistics(dev):
    from emoasr_amd import ops
    B, T, p = 64, 211, 0.1
    m0 = ops.las_dropmask(B, T, p, 1234, 0, dev).cpu()
    m1 = ops.las_dropmask(B, T, p, 1234, 1, dev).cpu()
    share, sd = m0.float().mean().item(), (p * (1 - p) / (B * T)) ** 0.5
    print(f"las_dropmask: kept share {share:.5f} (0.9 +- {4 * sd:.5f})")
    assert abs(share - (1 - p)) <= 4 * sd, share
    assert not torch.equal(m0, m1)
    assert torch.equal(m0, ops.las_dropmask(B, T, p, 1234, 0, dev).cpu())
    assert ops.las_dropmask(B, T, 0.0, 1234, 0, dev).all()


def test_model_with_attention_dropout(dev, fx):
    """train mode drops the attention weights with the hard-coded p = 0.1: the loss moves off the p = 0 golden, stays finite, and two
    engine steps (different counter values) draw different masks"""
    g = fx[2]
    model = _model(fx, dev, torch.float32)
    model.decoder.score.dropout_attn_rate = 0.1
    losses = []
    for _ in range(2):
        model.engine().step_count += 1
        model.zero_grad()
        loss, _, _, deouts = _run(model, g, "a", dev)
        assert torch.isfinite(loss) and torch.isfinite(deouts).all()
        losses.append(loss.item())
    ref = g["a/loss_total"].item()
    assert all(abs(v - ref) > 1e-4 * ref for v in losses) and losses[0] != losses[1], (losses, ref)
    model.eval()
    with torch.no_grad():   # eval: no dropout, the golden again
        loss, _, _ = model.decoder(g["a/eouts"].to(dev), g["a/elens"], None, g["a/ys"], g["a/ylens"], g["a/ys_in"], g["a/ys_out"])
    assert abs(loss.item() - ref) < 1e-3 * ref


# ---- decoding ----------------------------------------------------------------------------------------------------------------
_DECODE = [(1, 0.0), (1, 0.1), (4, 0.0), (4, 0.1)]


def _golden_nbest(g, b, bw, lw):
    key = f"decode/{b}/bw{bw}_lw{lw}"
    return las_ref_split(g[key + "/hyps"], g[key + "/lens"]), g[key + "/scores"].tolist()


def las_ref_split(flat, lens):
    from tests.util import split_ragged
    return split_ragged(flat, lens)


@pytest.mark.parametrize("bw,lw", _DECODE)
def test_beam_search_f32(dev, fx, bw, lw):
    g = fx[2]
    model = _model(fx, dev, torch.float32, train=False)
    for b in range(3):
        eo = g[f"decode/{b}/eouts"][None].to(dev)
        hyps, scores, logits, aligns = model.decoder.decode(eo, torch.tensor([eo.shape[1]]), None, bw, lw, lm=None, lm_weight=0.3)
        want, wscores = _golden_nbest(g, b, bw, lw)
        assert logits is None and aligns is None
        assert hyps == want, (b, hyps, want)
        assert all(abs(s - w) <= 1e-3 * abs(w) for s, w in zip(scores, wscores)), (scores, wscores)


@pytest.mark.parametrize("bw,lw", _DECODE)
def test_beam_search_bf16(dev, fx, bw, lw):
    """bf16 moves every log-probability by more than the 1e-3 decision margin the fixture's maker asserts, so bf16 is compared only
    where that margin decides nothing: every case is searched; beam 1 (recorded margins of 4.6 and more) must give the reference's
    hypothesis, beam 4 the reference's BEST hypothesis first; the best score within the bf16 loss bar (2e-2)"""
    g = fx[2]
    model = _model(fx, dev, torch.bfloat16, train=False)
    for b in range(3):
        eo = g[f"decode/{b}/eouts"][None].to(dev)
        hyps, scores, _, _ = model.decoder.decode(eo, torch.tensor([eo.shape[1]]), None, bw, lw)
        want, wscores = _golden_nbest(g, b, bw, lw)
        assert hyps and hyps[0] == want[0], (b, hyps, want)
        assert abs(scores[0] - wscores[0]) <= 2e-2 * abs(wscores[0]) + 2e-2, (scores, wscores)


def test_ctc_greedy_and_endless_search(dev, fx):
    g = fx[2]
    model = _model(fx, dev, torch.float32, train=False)
    eo = g["decode/0/eouts"][None].to(dev)
    el = torch.tensor([eo.shape[1]])
    a = model.decoder.decode(eo, el, None, 4, 0.0, decode_ctc_weight=1)
    model.decoder.ctc._owner = model.decoder._owner
    b = model.decoder.ctc.decode(eo, el, beam_width=1)
    assert a[0] == b[0] and len(a[0]) == 1
    with torch.no_grad():
        model.decoder.output.bias[fx[0]["eos_id"]] = -1e4   # <eos> never wins: the search runs out of steps
    model.engine().arena.refresh_shadow()
    assert model.decoder.decode(eo, el, None, 4, 0.0) == ([], [], None, None)
    assert model.decoder.decode(eo, el, None, 1, 0.1) == ([], [], None, None)


# ---- padding, end to end -------------------------------------------------------------------------------------------------------
def test_padding_is_ignored(dev, fx):
    g = fx[2]
    model = _model(fx, dev, torch.float32)
    loss0, _, _, _ = _run(model, g, "a", dev)
    gen = torch.Generator().manual_seed(5)
    eouts = torch.cat([g["a/eouts"], 50.0 * torch.randn(4, 6, 128, generator=gen)], dim=1)
    for b, n in enumerate(g["a/elens"].tolist()):
        eouts[b, n:] = 50.0 * torch.randn(eouts.shape[1] - n, 128, generator=gen)
    pad = torch.randint(3, 40, (4, 3), generator=gen)
    ys_in, ys_out = torch.cat([g["a/ys_in"], pad], 1), torch.cat([g["a/ys_out"], pad], 1)
    for b, n in enumerate(g["a/ylens"].tolist()):
        ys_in[b, n + 1:] = 7
        ys_out[b, n + 1:] = 9
    loss1, _, _ = model.decoder(eouts.to(dev), g["a/elens"], None, g["a/ys"], g["a/ylens"], ys_in, ys_out)
    print(f"las padding: {loss0.item():.7f} / {loss1.item():.7f}")
    assert abs(loss0.item() - loss1.item()) <= 1e-5 * abs(loss0.item())


def _batch():
    from tests.util import load_golden
    _, _, g3 = load_golden("l3_tiny")
    return {k: g3[k] for k in ("xs", "xlens", "ys", "ylens", "ys_in", "ys_out")}


@pytest.mark.parametrize("mode", _MODES[:2], ids=_MODE_IDS[:2])
def test_end_to_end_against_golden(dev, fx, mode):
    g = fx[2]
    model = _model(fx, dev, mode, encoder=True)
    d = _batch()
    loss, ld = model(d["xs"].to(dev), d["xlens"], d["ys"], d["ylens"], d["ys_in"], d["ys_out"])
    loss.backward()
    _check_losses(ld, g, "e2e", mode, ("loss_att", "loss_ctc"))
    names = [k[len("e2e/grad/"):] for k in g if k.startswith("e2e/grad/")]
    assert len(names) == 3
    params = dict(model.named_parameters())
    for n in names:
        ref, got = g["e2e/grad/" + n], params[n].grad.float().cpu()
        cos = torch.nn.functional.cosine_similarity(got.flatten().double(), ref.flatten().double(), dim=0).item()
        err = ((got - ref).abs().max() / ref.abs().max()).item()
        print(f"las e2e {n} {mode}: max-error {err:.3e}, cosine {cos:.8f}")
        if mode == torch.bfloat16:
            assert cos > 0.98, (n, cos)
        else:
            assert err < 5e-3 and cos >= 0.9999, (n, err, cos)


def test_train_step_and_test_step(dev, fx):
    from emoasr_amd.decode import test_step as decode_step
    from emoasr_amd.optimizers import Adam
    from emoasr_amd.train import train_step
    cfg, _, g = fx
    model = _model(fx, dev, torch.float32, train=False, encoder=True)
    d = _batch()
    n = int(d["xlens"][0])
    data = {"utt_ids": ["utt0"], "texts": ["ref"], "xs": d["xs"][0:1, :n], "xlens": d["xlens"][0:1]}
    utt, hyps, scores, ref = decode_step(model, data, 4, 0.0, 0.0, False, None, 0.0, dev)
    assert (utt, ref) == ("utt0", "ref") and hyps[0] == g["e2e/hyp"].tolist()
    assert abs(scores[0] - g["e2e/score"].item()) <= 1e-3 * abs(g["e2e/score"].item())
    params = SimpleNamespace(**dict(las_ref.las_asr_config(cfg), accum_grad=1, clip_grad_norm=5.0))
    # a step small enough for first-order descent: Adam's first step moves every parameter by lr whatever the gradient's size, and
    # this decoder sits in a sharp minimum of these utterances (measured: lr 1e-3 gives 11.14 -> 43.8, 1e-4 11.14 -> 11.27 -> 10.26,
    # 1e-5 11.14 -> 11.05 -> 10.98 -> 10.91)
    optimizer = Adam(model.parameters(), lr=1e-5)
    model.train()
    first = train_step(model, optimizer, d, params, dev)["loss_total"]
    assert abs(first - g["e2e/loss_total"].item()) < 1e-3 * first
    second = train_step(model, optimizer, d, params, dev)["loss_total"]   # (train mode again: eval would swap the BatchNorm statistics)
    print(f"las train_step: {first:.4f} -> {second:.4f}")
    assert second < first, (second, first)


def test_rnn_encoder_trains(dev, fx):
    """the LAS decoder under the RNN encoder of rnn_att_tiny (no golden for this pair): a finite, decreasing loss over 5 steps"""
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.optimizers import Adam
    from emoasr_amd.train import train_step
    from tests.rnn_util import load_rnn_golden
    rcfg, rsd, rg = load_rnn_golden("rnn_att_tiny")
    cfg = dict(vars(rcfg), **fx[0], decoder_type="las", accum_grad=1, clip_grad_norm=5.0)
    params = SimpleNamespace(**cfg)
    torch.manual_seed(0)
    model = ASR(params, compute_dtype=torch.bfloat16)
    model.load_state_dict({k: v for k, v in rsd.items() if k.startswith("encoder.")}, strict=False)
    model.load_state_dict(fx[1], strict=False)
    optimizer = Adam(model.parameters(), lr=1e-3)
    model.to(dev).train()
    data = {k: rg[k] for k in ("xs", "xlens", "ys", "ylens", "ys_in", "ys_out")}
    losses = [train_step(model, optimizer, data, params, dev)["loss_total"] for _ in range(5)]
    assert all(torch.isfinite(torch.tensor(losses))), losses
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
