"""The RNN LM fused inside the batched joint CTC / attention search (decoder.joint_rnnlm_impl = "device"): the
step kernel over R rows bit for bit against emoasr_rnnlm_step, and the search end to end on l3_tiny + rnnlm_tiny against the default
host search per utterance, the reference's outputs (tests/golden/rnnlm_tiny.npz) and the per-cell batched search (the grid).

Bars: hypotheses exact and scores within 1e-4 between the two f32 forms (the bar tests/test_joint_beam_batch_gpu.py holds between the
batched and the single search), 1e-3 against the fixture (tests/test_rnnlm_beam_gpu.py); the step at 70 rows against f64 at the bars of
tests/test_rnnlm_gpu.py::test_step_edges (1e-4 of range in f32, 6e-2 in bf16); bf16 end to end 2e-2 |s| + 1e-3 (test_batch_bf16)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rnnlm_ref as ref
from tests.rnnlm_util import RNNLM_CFG, rnnlm_golden, rnnlm_state
from tests.util import CONFIGS, DECODE_SETTINGS, load_golden, split_ragged

pytestmark = pytest.mark.gpu
JOINT_SETTINGS = [si for si, st in enumerate(DECODE_SETTINGS) if st["lm_weight"] > 0]
CUT_FRAC = (0.6, 0.6)


def _rel(a, b):
    return ((a.double().cpu() - b.double()).abs().max() / (b.double().abs().max() + 1e-12)).item()


# =========================================================================================== 1. the step kernel, bit for bit
STEP_CASES = [("f32", torch.float32, (2, 48, 64)), ("f32x3", "f32x3", (2, 48, 64)), ("bf16-mfma", torch.bfloat16, (2, 64, 64)),
              ("bf16-valu", torch.bfloat16, (2, 48, 64))]
_LMS = {}


def _step_lm(name, dtype, shape, dev):
    if name not in _LMS:
        from emoasr_amd import ops
        from emoasr_amd.modeling.lm import LM
        L, E, H = shape
        V = 40
        sd64 = ref.random_state(V, E, H, L, seed=7 + E + H, out_scale=4.0)
        lm = LM(SimpleNamespace(**dict(RNNLM_CFG, vocab_size=V, embedding_size=E, hidden_size=H, num_layers=L)), compute_dtype=dtype)
        lm.load_state_dict({k: v.float() for k, v in sd64.items()})
        lm = lm.to(dev).eval()
        A = lm._prepare()
        ws = [lm._w(l) for l in range(L)]
        W = ops.RnnlmStepWeights(A.w("lm.embed.weight"), [w[0] for w in ws], [w[1] for w in ws], lm._bias, A.w("lm.output.weight"),
                                 A.p("lm.output.bias"))
        sdr = {n: (A.p(n) if "bias" in n else A.w(n)).detach().double().cpu() for n in sd64}      # what the device holds, in f64
        _LMS[name] = (lm, W, sdr)
    return _LMS[name]


@pytest.mark.parametrize("R", [1, 15, 16, 17, 32, 33, 70])
@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_step_rows_equals_the_step_bit_for_bit(dev, case, R):
    """emoasr_rnnlm_step_rows on a pool of 2 R slots against emoasr_rnnlm_step run in chunks of at most 32 rows with the same sources
    and destinations: the destination half of ph / pc equal bit for bit, the source half and everything else unchanged, the raw
    logits equal bit for bit where both heads ran on the same number of rows (R <= 32); R = 70 also against f64"""
    from emoasr_amd import ops
    name, dtype, (L, E, H) = case
    lm, W, sdr = _step_lm(name, dtype, (L, E, H), dev)
    V, ld = W.V, W.V + 4
    es = 2 if lm.compute_dtype == torch.bfloat16 else 4
    assert ops.rnnlm_step_rows_supported(torch.empty(0, device=dev, dtype=lm.compute_dtype), L, E, H)
    for src_base in (0, R):
        dst_base = R - src_base
        gen = torch.Generator().manual_seed(100 * R + src_base)
        ph0 = torch.randn(L, 2 * R, H, generator=gen).mul(0.5).to(lm.compute_dtype).to(dev)
        pc0 = torch.randn(L, 2 * R, H, generator=gen).to(dev)
        lg0 = torch.randn(R + 1, ld, generator=gen).to(dev)
        ids = torch.randint(0, V, (R,), generator=gen)
        parent = torch.randint(0, R, (R,), generator=gen)
        parent[::3] = parent[0]                     # children of one parent
        if R > 32:
            parent[0], parent[R - 1] = R - 1, 0     # parents in another tile
        if R >= 2:
            parent[1] = R                           # out of range: the zero state
        if R >= 3:
            parent[2] = -1
        if R == 1 and src_base:
            parent[0] = 5
        live = (parent >= 0) & (parent < R)
        src = torch.where(live, src_base + parent, torch.full_like(parent, -1))
        dst = dst_base + torch.arange(R)
        to_dev = lambda t: t.to(torch.int32).to(dev)
        ids_d, par_d, src_d, dst_d = to_dev(ids), to_dev(parent), to_dev(src), to_dev(dst)
        with torch.no_grad(), ops.stream_scope(lm._split()):
            # the reference: today's step, at most 32 rows a call; its raw logits stay in its workspace behind the h rows
            ph_r, pc_r = ph0.clone(), pc0.clone()
            logp = torch.zeros(32, V, device=dev)
            lg_r = torch.zeros(R, V, device=dev)
            off = (32 * H * es + 255) // 256 * 256
            for i0 in range(0, R, 32):
                n = min(32, R - i0)
                ops.rnnlm_step(W, n, ids_d[i0:], ph_r, pc_r, src_d[i0:], dst_d[i0:], logp)
                lg_r[i0:i0 + n] = W.ws[off:off + n * V * 4].view(torch.float32).view(n, V)
            ph, pc, lg = ph0.clone(), pc0.clone(), lg0.clone()
            ops.rnnlm_step_rows(W, R, ids_d, par_d, ph, pc, src_base, dst_base, lg)
        torch.cuda.synchronize()
        d = slice(dst_base, dst_base + R)
        s = slice(src_base, src_base + R)
        assert torch.equal(ph[:, d], ph_r[:, d]) and torch.equal(pc[:, d], pc_r[:, d]), (name, R, src_base)
        assert not torch.equal(ph[:, d], ph0[:, d])
        assert torch.equal(ph[:, s], ph0[:, s]) and torch.equal(pc[:, s], pc0[:, s]), "the source half changed"
        assert torch.equal(lg[R:], lg0[R:]) and torch.equal(lg[:, V:], lg0[:, V:]), "logits written outside [R][V]"
        assert torch.isfinite(lg[:R, :V]).all()
        if R <= 32:
            assert torch.equal(lg[:R, :V], lg_r), (name, R, src_base)
        if R == 70:
            h_in = ph0.double().cpu()[:, src.clamp(min=0)] * live.double().view(1, R, 1)
            c_in = pc0.double().cpu()[:, src.clamp(min=0)] * live.double().view(1, R, 1)
            out, (want_h, want_c) = ref.lstm_stack(sdr, sdr["lm.embed.weight"][ids].unsqueeze(1), (h_in, c_in))
            want_lg = out[:, 0] @ sdr["lm.output.weight"].t() + sdr["lm.output.bias"]
            errs = (_rel(lg[:R, :V], want_lg), _rel(ph[:, d], want_h), _rel(pc[:, d], want_c), _rel(lg_r, want_lg))
            print(f"step_rows {name} R={R} src_base={src_base}: logits / h / c {errs[:3]} of range (the chunked step's logits {errs[3]:.3e})")
            assert max(errs[:3]) < (6e-2 if lm.compute_dtype == torch.bfloat16 else 1e-4), errs


def test_step_rows_refusals(dev):
    from emoasr_amd import lib, ops
    lm, W, _ = _step_lm(*STEP_CASES[0], dev)
    R = 4
    ph, pc = torch.zeros(2, 2 * R, 64, device=dev), torch.zeros(2, 2 * R, 64, device=dev)
    lg = torch.zeros(R, 40, device=dev)
    z = torch.zeros(R, dtype=torch.int32, device=dev)
    for sb, db in ((0, 0), (0, 3), (5, 0), (-1, 4), (0, 5)):      # overlapping halves, halves outside the pools
        with pytest.raises(lib.EmoasrHipError, match="source slots"):
            ops.rnnlm_step_rows(W, R, z, z, ph, pc, sb, db, lg)
    torch.cuda.synchronize()
    assert not ph.any() and not pc.any() and not lg.any()


# =========================================================================================== 2-7. end to end on l3_tiny + rnnlm_tiny
_CACHE = {}


def _models(dtype, dev):
    key = ("model", dtype, str(dev))
    if key not in _CACHE:
        from emoasr_amd.modeling.asr import ASR
        from emoasr_amd.modeling.lm import LM
        cfg, sd, g = load_golden("l3_tiny")
        model = ASR(SimpleNamespace(**CONFIGS["l3_tiny"]), compute_dtype=dtype)
        model.load_state_dict(sd)
        lm = LM(SimpleNamespace(**RNNLM_CFG), compute_dtype=dtype)
        lm.load_state_dict(rnnlm_state(rnnlm_golden()))
        _CACHE[key] = (model.to(dev).eval(), lm.to(dev).eval(), g)
    return _CACHE[key]


def _five(dtype, dev):
    """-> (eouts [5, Tmax, d], elens): utterance 0, utterance 1, both cut to CUT_FRAC of their frames, utterance 1 cut to one"""
    key = ("five", dtype, str(dev))
    if key not in _CACHE:
        model, _, g = _models(dtype, dev)
        enc = []
        with torch.no_grad():
            for b in range(2):
                n = int(g["xlens"][b])
                e, el, _ = model.encoder(g["xs"][b:b + 1, :n].to(dev), g["xlens"][b:b + 1])
                enc.append(e[0, :int(el[0])])
        parts = [enc[0], enc[1], enc[0][:max(2, round(CUT_FRAC[0] * enc[0].shape[0]))],
                 enc[1][:max(2, round(CUT_FRAC[1] * enc[1].shape[0]))], enc[1][:1]]
        elens = [p.shape[0] for p in parts]
        eouts = torch.zeros(5, max(elens), parts[0].shape[1], device=dev, dtype=parts[0].dtype)
        for b, p in enumerate(parts):
            eouts[b, :elens[b]] = p
        _CACHE[key] = (eouts, elens)
    return _CACHE[key]


def _single(dtype, dev, kw):
    """the default host search (joint_rnnlm_impl = "host", one joint_beam_search per utterance) on the five, once per setting"""
    key = ("single", dtype, str(dev), tuple(sorted(kw.items())))
    if key not in _CACHE:
        model, lm, _ = _models(dtype, dev)
        eouts, elens = _five(dtype, dev)
        dec = model.decoder
        assert dec.joint_beam_impl == "single" and dec.joint_rnnlm_impl == "host"
        _CACHE[key] = [dec.decode(eouts[b:b + 1, :elens[b]], [elens[b]], None, lm=lm, **kw)[:2] for b in range(5)]
    return _CACHE[key]


def _watch(monkeypatch, lm):
    """-> (chunks, steps): the calls of _batch_search_chunk as (utterances, grid argument) and of lm.step"""
    from emoasr_amd.modeling import beam_search_device as bsd
    chunks, steps = [], []
    orig = bsd._batch_search_chunk
    monkeypatch.setattr(bsd, "_batch_search_chunk", lambda *a, **k: (chunks.append((len(a[3]), k.get("grid"), a[6] is not None)), orig(*a, **k))[1])
    orig_step = lm.step
    monkeypatch.setattr(lm, "step", lambda *a, **k: (steps.append(1), orig_step(*a, **k))[1])
    return chunks, steps


def _close(a, b, tol=1e-4):
    return len(a) == len(b) and all(abs(x - y) < tol for x, y in zip(a, b))


@pytest.mark.parametrize("len_weight", [0.0, 0.3])
@pytest.mark.parametrize("si", JOINT_SETTINGS)
def test_batch_equals_the_single_search_f32(dev, si, len_weight, monkeypatch):
    """decoder.decode on the batch of five under joint_rnnlm_impl = "device" equals the default host search on eouts[b:b+1, :elens[b]]:
    hypotheses in order, scores within 1e-4; the single search's neighbouring scores differ by more than 1e-3 (the oracle search
    driven by tests/rnnlm_ref.py on the CPU: smallest gap 0.077 at utterance 3 under setting 2, at least 0.59 elsewhere; the one-frame
    utterance rests on this assert alone); utterances 0 and 1 at the setting's own len_weight also equal the reference's outputs.
    One chunk, and lm.step is never called."""
    model, lm, _ = _models(torch.float32, dev)
    eouts, elens = _five(torch.float32, dev)
    kw = dict(DECODE_SETTINGS[si], len_weight=len_weight)
    want = _single(torch.float32, dev, kw)
    for b, (h, s) in enumerate(want):
        gaps = [a - c for a, c in zip(s, s[1:])]
        print(f"setting {si} len_weight {len_weight} search {b} (T {elens[b]}): {len(h)} results, smallest score gap "
              f"{min(gaps) if gaps else float('nan'):.4g}")
        assert all(d > 1e-3 for d in gaps), (si, len_weight, b, s)
    chunks, steps = _watch(monkeypatch, lm)
    monkeypatch.setattr(model.decoder, "joint_rnnlm_impl", "device")
    hyps, scores, _, _ = model.decoder.decode(eouts, elens, None, lm=lm, **kw)
    assert chunks == [(5, None, True)] and steps == []
    assert len(hyps) == 5 and len(scores) == 5
    for b in range(5):
        assert hyps[b] == want[b][0], (si, len_weight, b, hyps[b], want[b][0])
        assert _close(scores[b], want[b][1]), (si, len_weight, b, scores[b], want[b][1])
    assert sum(len(h) for h in hyps) >= 5
    if len_weight == DECODE_SETTINGS[si]["len_weight"]:
        g = rnnlm_golden()
        for b in range(2):
            assert hyps[b] == split_ragged(g[f"joint/{si}/{b}/hyps"], g[f"joint/{si}/{b}/lens"]), (si, b)
            np.testing.assert_allclose(scores[b], g[f"joint/{si}/{b}/scores"].numpy(), rtol=0, atol=1e-3)


def test_one_utterance_through_the_batched_search(dev, monkeypatch):
    """joint_beam_impl = "batch" + joint_rnnlm_impl = "device": one utterance takes the batched search with the LM on the device and
    returns the single search's shape and results"""
    model, lm, _ = _models(torch.float32, dev)
    eouts, elens = _five(torch.float32, dev)
    kw = dict(DECODE_SETTINGS[2])
    want = _single(torch.float32, dev, kw)
    chunks, steps = _watch(monkeypatch, lm)
    monkeypatch.setattr(model.decoder, "joint_beam_impl", "batch")
    monkeypatch.setattr(model.decoder, "joint_rnnlm_impl", "device")
    for b in (0, 4):
        hyps, scores, _, _ = model.decoder.decode(eouts[b:b + 1, :elens[b]], [elens[b]], None, lm=lm, **kw)
        assert hyps == want[b][0] and _close(scores, want[b][1]), (b, hyps, want[b])
    assert chunks == [(1, None, True)] * 2 and steps == []


def test_chunking(dev, monkeypatch):
    """with a chunk capacity of two searches the batch of five returns what it returns in one chunk"""
    from emoasr_amd.modeling import beam_search_device as bsd
    model, lm, _ = _models(torch.float32, dev)
    eouts, elens = _five(torch.float32, dev)
    kw = dict(DECODE_SETTINGS[2])
    monkeypatch.setattr(model.decoder, "joint_rnnlm_impl", "device")
    whole = model.decoder.decode(eouts, elens, None, lm=lm, **kw)
    chunks, steps = _watch(monkeypatch, lm)
    monkeypatch.setattr(bsd, "batch_chunk_capacity", lambda *a, **k: 2)
    parts = model.decoder.decode(eouts, elens, None, lm=lm, **kw)
    assert [c[0] for c in chunks] == [2, 2, 1] and steps == []
    assert parts[0] == whole[0]
    for a, c in zip(parts[1], whole[1]):
        assert _close(a, c), (a, c)


def test_replayed_graphs_outlive_a_collection(dev):
    """the fused chunk of B = 3, elens (9, 4, 2), W = 4 is captured on one set of frames; after gc.collect() the same graphs are
    replayed on other frames of the same shape and return exactly what a fresh engine, which captures anew, returns for them:
    everything the captured launches point at (structs, pointer tables, workspaces) is still alive"""
    import gc
    from emoasr_amd.modeling import beam_search_device as bsd
    from emoasr_amd.modeling.asr import ASR
    model, lm, _ = _models(torch.float32, dev)
    five, five_lens = _five(torch.float32, dev)
    elens = [9, 4, 2]
    assert min(five_lens[:2]) >= 9 and five_lens[3] >= 2
    first, second = five[[0, 1, 2], :9].contiguous(), five[[1, 0, 3], :9].contiguous()
    run = lambda dec, frames: bsd._batch_search_chunk(dec, bsd._engine_of(dec), frames, elens, 4, 0.0, lm, 0.3, 0.3)
    run(model.decoder, first)
    eng = bsd._engine_of(model.decoder)
    graphs = eng._beam_batch_bufs[1].graphs[1]
    gc.collect()
    got = run(model.decoder, second)
    assert eng._beam_batch_bufs[1].graphs[1] is graphs, "the second call replays the first call's graphs"
    fresh = ASR(SimpleNamespace(**CONFIGS["l3_tiny"]), compute_dtype=torch.float32)
    fresh.load_state_dict(load_golden("l3_tiny")[1])
    want = run(fresh.to(dev).eval().decoder, second)
    assert got == want, (got, want)
    assert all(len(h) >= 1 for h in got[0]) and got != run(model.decoder, first)


@pytest.mark.parametrize("ctc_weight,W,lm_weights,len_weights", [(0.3, 4, [0.0, 0.3], [0.0, 0.1, 0.3]), (0.0, 3, [0.5], [0.0, 0.2, 0.3])])
def test_grid(dev, ctc_weight, W, lm_weights, len_weights, monkeypatch):
    """every cell of joint_beam_search_device_grid equals the batched device search run with that cell's weights (hypotheses exact,
    scores within 1e-4); cells of one lm_weight come from ONE search; the lm_weight = 0 cells are the search without an LM"""
    from emoasr_amd.modeling import beam_search_device as bsd
    model, lm, _ = _models(torch.float32, dev)
    eouts, elens = _five(torch.float32, dev)
    dec = model.decoder
    monkeypatch.setattr(dec, "joint_rnnlm_impl", "device")
    per_cell = []
    for a in lm_weights:
        for w in len_weights:
            per_cell.append(bsd.joint_beam_search_device_batch(dec, eouts, elens, W, w, lm if a > 0 else None, a, ctc_weight)[:2])
    chunks, steps = _watch(monkeypatch, lm)
    hyps, scores = bsd.joint_beam_search_device_grid(dec, eouts, elens, W, lm, lm_weights, len_weights, ctc_weight)
    assert steps == []
    positive = [a for a in lm_weights if a > 0]
    expect = ([(5, None, False)] if len(positive) < len(lm_weights) else [])
    assert [c for c in chunks if c[1] is None] == expect
    grids = [c for c in chunks if c[1] is not None]
    assert len(grids) == 1 and grids[0][0] == 5 and grids[0][2]
    sutt, mus, _ = grids[0][1]
    assert list(sutt) == [b for b in range(5) for _ in positive] and list(mus) == positive * 5
    for b in range(5):
        assert len(hyps[b]) == len(per_cell)
        for c, (h, s) in enumerate(per_cell):
            assert hyps[b][c] == h[b], (b, c, hyps[b][c], h[b])
            assert _close(scores[b][c], s[b]), (b, c, scores[b][c], s[b])
    assert sum(len(h) for cells in hyps for h in cells) >= len(per_cell) * 4


def test_batch_bf16(dev, monkeypatch):
    """bf16: the batch runs, scores finite and sorted; the best hypothesis equals the bf16 host search's, its score within the bf16 bar
    of tests/test_joint_beam_batch_gpu.py::test_batch_bf16.  An utterance whose f32 host search puts its two best results closer than
    that bar is left out of the hypothesis comparison and printed; at most one of the five"""
    model, lm, _ = _models(torch.bfloat16, dev)
    eouts, elens = _five(torch.bfloat16, dev)
    kw = dict(DECODE_SETTINGS[2])
    want = _single(torch.bfloat16, dev, kw)
    f32 = _single(torch.float32, dev, kw)
    chunks, steps = _watch(monkeypatch, lm)
    monkeypatch.setattr(model.decoder, "joint_rnnlm_impl", "device")
    hyps, scores, _, _ = model.decoder.decode(eouts, elens, None, lm=lm, **kw)
    assert chunks == [(5, None, True)] and steps == []
    left_out = []
    for b in range(5):
        assert all(np.isfinite(scores[b])) and scores[b] == sorted(scores[b], reverse=True), (b, scores[b])
        assert all(0 < v < 40 for h in hyps[b] for v in h)
        if not want[b][0]:
            continue
        s32 = f32[b][1]
        if len(s32) >= 2 and s32[0] - s32[1] < 2e-2 * abs(s32[0]) + 1e-3:
            print(f"bf16 search {b}: left out, the f32 search's two best are {s32[0]:.5f} and {s32[1]:.5f}")
            left_out.append(b)
            continue
        print(f"bf16 search {b}: best score {scores[b][0]:.5f}, host search {want[b][1][0]:.5f}")
        assert hyps[b][0] == want[b][0][0], (b, hyps[b], want[b][0])
        assert abs(scores[b][0] - want[b][1][0]) < 2e-2 * abs(want[b][1][0]) + 1e-3, (b, scores[b][0], want[b][1][0])
    assert len(left_out) <= 1, left_out


def test_refusals_under_device_and_the_default(dev, monkeypatch):
    from emoasr_amd.modeling.lm import LM
    model, lm, _ = _models(torch.float32, dev)
    eouts, elens = _five(torch.float32, dev)
    dec = model.decoder
    e3, l3 = eouts[:3], elens[:3]
    kw = dict(DECODE_SETTINGS[2])
    chunks, steps = _watch(monkeypatch, lm)
    # the default: the RNN LM takes the host search per utterance
    assert dec.joint_rnnlm_impl == "host"
    dec.decode(e3, l3, None, lm=lm, **kw)
    assert chunks == [] and len(steps) >= 3
    monkeypatch.setattr(dec, "joint_rnnlm_impl", "device")
    wide = LM(SimpleNamespace(**dict(RNNLM_CFG, vocab_size=RNNLM_CFG["vocab_size"] + 8)), compute_dtype=torch.float32).to(dev).eval()
    with pytest.raises(ValueError, match="vocabulary"):
        dec.decode(e3, l3, None, lm=wide, **kw)
    _, lm16, _ = _models(torch.bfloat16, dev)
    with pytest.raises(ValueError, match="computes in"):
        dec.decode(e3, l3, None, lm=lm16, **kw)
    with pytest.raises(ValueError, match="beam_width 33"):
        dec.decode(e3, l3, None, lm=lm, **dict(kw, beam_width=33))
    assert chunks == []
    monkeypatch.setattr(dec, "joint_rnnlm_impl", "both")
    with pytest.raises(ValueError, match="joint_rnnlm_impl"):
        dec.decode(e3, l3, None, lm=lm, **kw)
